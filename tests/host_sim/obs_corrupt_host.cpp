// TEST INFRASTRUCTURE ONLY: the per-element body of the observation corruption (wheeledlab_amd/csrc/wl_obs_corrupt_dev.h: the table
// check, the packed term, the draws, the lane that reads four columns, draws, stores its bias elements and clips and scales) compiled
// for the host through the stand-in hip_runtime.h, as a stand-alone program that tests/test_obs_corrupt_cpu.py holds against the
// reference without a GPU -- and the place for -fsanitize=address,undefined runs of that code.  Every buffer is allocated at its exact
// size, so an index the lane gets wrong is an out-of-bounds access the sanitizer reports.
//
//   obs_corrupt_host IN OUT
// IN : int64 n, D, obs_stride, out_stride, n_terms, has_reset_b, state_rows, state_stride, enable, in_place; uint64 seed, step,
//      env_offset; WlObsCorruptTerm table[n_terms]; uint32 obs[n][obs_stride]; uint32 state[state_rows][state_stride]; float
//      bias[n][Db]; uint8 reset_a[n]; uint8 reset_b[n] (if has_reset_b)
// OUT: int64 Db (or -1 and nothing else: the table was refused); uint32 out[n][out_stride] (columns beyond D keep 0xDEADBEEF; in place:
//      the obs buffer); float bias[n][Db]; uint8 writes[n][out_stride] (times each word was produced: 1 below D, 0 beyond)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "wl_obs_corrupt_dev.h"

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
    int64_t h[10];
    uint64_t key[3];
    if (!rd(f, h, 10) || !rd(f, key, 3)) return 4;
    const int64_t n = h[0], D = h[1], obs_stride = h[2], out_stride = h[3], n_terms = h[4], has_b = h[5], state_rows = h[6], state_stride = h[7],
                  enable = h[8], in_place = h[9];
    if (n < 1 || n_terms < 0 || n_terms > 1024 || obs_stride < D || out_stride < D || state_rows < 0 || (state_rows > 0 && state_stride < n)) return 5;
    if (in_place && obs_stride != out_stride) return 5;
    std::vector<WlObsCorruptTerm> t(n_terms);
    if (!rd(f, t.data(), t.size())) return 4;
    const int64_t Db = obscorrupt_width(t.data(), (int)n_terms, (int)D);
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 3;
    if (Db < 0) {
        const int64_t bad = -1;
        const bool ok = wr(g, &bad, 1);
        return fclose(g) == 0 && ok ? 0 : 6;
    }
    for (const WlObsCorruptTerm& q : t)
        if (q.state_row >= 0 && (int64_t)q.state_row + q.width > state_rows) return 5;
    std::vector<uint32_t> obs(n * obs_stride), state(state_rows * state_stride), own(in_place ? 0 : n * out_stride, 0xDEADBEEFu);
    std::vector<float> bias(n * Db);
    std::vector<uint8_t> ra(n), rb(has_b ? n : 0), writes(n * out_stride, 0);
    if (!rd(f, obs.data(), obs.size()) || !rd(f, state.data(), state.size()) || !rd(f, bias.data(), bias.size()) || !rd(f, ra.data(), ra.size()) ||
        !rd(f, rb.data(), rb.size()))
        return 4;
    fclose(f);
    std::vector<uint32_t>& out = in_place ? obs : own;
    std::vector<ObsCorruptDevTerm> dt(n_terms);
    for (int64_t k = 0; k < n_terms; ++k) dt[k] = obscorrupt_pack(t[k]);
    ObsCorruptArgs a{};
    a.obs = obs.data();
    a.state = state_rows ? state.data() : nullptr;
    a.bias = Db ? bias.data() : nullptr;
    a.reset_a = ra.data();
    a.reset_b = has_b ? rb.data() : nullptr;
    a.obs_stride = obs_stride;
    a.state_stride = state_stride;
    a.seed = key[0];
    a.step = key[1];
    a.env0 = (uint32_t)key[2];
    a.n = (int32_t)n;
    a.D = (int32_t)D;
    a.Db = (int32_t)Db;
    a.n_terms = (int32_t)n_terms;
    a.nblk = (int32_t)((D + OBSCORRUPT_SLOT - 1) / OBSCORRUPT_SLOT);
    a.lanes = (int32_t)(n * a.nblk);
    a.enable = enable != 0;
    for (int lane = 0; lane < a.lanes; ++lane) {
        const int e = lane / a.nblk, c0 = (lane - e * a.nblk) * OBSCORRUPT_SLOT;
        const int count = a.D - c0 < OBSCORRUPT_SLOT ? a.D - c0 : OBSCORRUPT_SLOT;
        uint32_t x[OBSCORRUPT_SLOT] = {0u, 0u, 0u, 0u}, v[OBSCORRUPT_SLOT] = {0u, 0u, 0u, 0u};
        for (int i = 0; i < count; ++i) x[i] = obs.at(e * obs_stride + c0 + i);
        obscorrupt_lane(e, c0, count, a, dt.data(), x, v);
        for (int i = 0; i < count; ++i) {
            out.at(e * out_stride + c0 + i) = v[i];
            ++writes.at(e * out_stride + c0 + i);
        }
    }
    const bool ok = wr(g, &Db, 1) && wr(g, out.data(), out.size()) && wr(g, bias.data(), bias.size()) && wr(g, writes.data(), writes.size());
    return fclose(g) == 0 && ok ? 0 : 6;
}
