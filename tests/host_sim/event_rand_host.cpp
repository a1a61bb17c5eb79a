// TEST INFRASTRUCTURE ONLY: the per-env body of the per-episode domain randomisation (wheeledlab_amd/csrc/wl_event_rand_dev.h: the
// table check, the packed term, the draws, the env that reads its flags and timers, applies its terms and stores what changed) compiled
// for the host through the stand-in hip_runtime.h, as a stand-alone program that tests/test_event_rand_cpu.py holds against the
// reference without a GPU -- and the place for -fsanitize=address,undefined runs of that code.  Every buffer is allocated at its exact
// size, so an index the body gets wrong is an out-of-bounds access the sanitizer reports.
//
//   event_rand_host IN OUT
// IN : int64 n, stride, n_terms, has_reset_b, has_mask, mask_terms, calls; uint64 seed, env_offset; WlEventRandTerm table[n_terms];
//      uint32 state[WL_S_COUNT][stride]; uint32 block[rows][stride]; then per call: uint64 step; double step_dt; uint8 reset_a[n];
//      uint8 reset_b[n] (if has_reset_b); uint8 mask[n] (if has_mask)
// OUT: int64 rows (or -1 and nothing else: the table was refused); after every call: uint32 state[WL_S_COUNT][stride]; uint32 block[rows][stride]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "wl_event_rand_dev.h"

namespace {
template <class T>
bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
bool wr(FILE* f, const T* p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int64_t h[7];
    uint64_t key[2];
    if (!rd(f, h, 7) || !rd(f, key, 2)) return 4;
    const int64_t n = h[0], stride = h[1], n_terms = h[2], has_b = h[3], has_mask = h[4], mask_terms = h[5], calls = h[6];
    if (n < 1 || stride < n || n_terms < 0 || n_terms > 1024 || calls < 0) return 5;
    std::vector<WlEventRandTerm> t(n_terms);
    if (!rd(f, t.data(), t.size())) return 4;
    const int64_t rows = eventrand_width(t.data(), (int)n_terms);
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 3;
    if (rows < 0) {
        const int64_t bad = -1;
        const bool ok = wr(g, &bad, 1);
        return fclose(g) == 0 && ok ? 0 : 6;
    }
    std::vector<float> state(WL_S_COUNT * stride);      // (words: read and written as they are)
    std::vector<uint32_t> block(rows * stride);
    std::vector<uint8_t> ra(n), rb(has_b ? n : 0), mask(has_mask ? n : 0);
    if (!rd(f, state.data(), state.size()) || !rd(f, block.data(), block.size())) return 4;
    std::vector<EventRandDevTerm> dt(n_terms);
    for (int64_t k = 0; k < n_terms; ++k) dt[k] = eventrand_pack(t[k]);
    bool ok = wr(g, &rows, 1);
    for (int64_t c = 0; c < calls; ++c) {
        uint64_t step;
        double step_dt;
        if (!rd(f, &step, 1) || !rd(f, &step_dt, 1) || !rd(f, ra.data(), ra.size()) || !rd(f, rb.data(), rb.size()) || !rd(f, mask.data(), mask.size()))
            return 4;
        EventRandArgs a{};
        a.state = state.data();
        a.block = block.data();
        a.reset_a = ra.data();
        a.reset_b = has_b ? rb.data() : nullptr;
        a.mask = has_mask ? mask.data() : nullptr;
        a.stride = stride;
        a.seed = key[0];
        a.step = step;
        a.step_dt = (float)step_dt;
        a.env0 = (uint32_t)key[1];
        a.mask_terms = (uint32_t)mask_terms;
        a.n = (int32_t)n;
        a.n_terms = (int32_t)n_terms;
        for (int e = 0; e < a.n; ++e) eventrand_env(e, a, dt.data());
        ok = ok && wr(g, state.data(), state.size()) && wr(g, block.data(), block.size());
    }
    fclose(f);
    return fclose(g) == 0 && ok ? 0 : 6;
}
