// TEST INFRASTRUCTURE ONLY: the index map of the observation-history push (wheeledlab_amd/csrc/wl_obs_history_dev.h: the table check,
// the term search, the walk along a 16-byte line and the source of every output) compiled for the host through the stand-in
// hip_runtime.h, as a stand-alone program that tests/test_obs_history_cpu.py holds against the reference without a GPU -- and the
// place for -fsanitize=address,undefined runs of that code.  Every buffer is allocated at its exact size, so an index the map gets
// wrong is an out-of-bounds access the sanitizer reports.
//
//   obs_history_host IN OUT
// IN : int64 n, D, obs_stride, n_terms, has_prev, has_reset_b, shift (0 .. 3: where `next` starts inside a 16-byte line);
//      int32 table[n_terms][4]; uint32 obs[n][obs_stride]; uint32 prev[n][Dh] (if has_prev); uint8 reset_a[n]; uint8 reset_b[n] (if
//      has_reset_b)
// OUT: int64 Dh (or -1 and nothing else: the table was refused); uint32 next[n][Dh]; uint8 writes[n][Dh] (times each output was
//      produced: all 1); int64 whole (slots stored as one 16-byte line)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "wl_obs_history_dev.h"

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
    if (!rd(f, h, 7)) return 4;
    const int64_t n = h[0], D = h[1], stride = h[2], n_terms = h[3], has_prev = h[4], has_b = h[5], shift = h[6];
    if (n < 1 || n_terms < 0 || n_terms > 1024 || shift < 0 || shift > 3 || stride < D) return 5;
    std::vector<WlObsHistoryTerm> t(n_terms);
    if (!rd(f, t.data(), t.size())) return 4;
    const int64_t Dh = obshist_width(t.data(), (int)n_terms, (int)D);
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 3;
    if (Dh < 0) {
        const int64_t bad = -1;
        const bool ok = wr(g, &bad, 1);
        return fclose(g) == 0 && ok ? 0 : 6;
    }
    std::vector<uint32_t> obs(n * stride), prev(has_prev ? n * Dh : 0), next(n * Dh, 0xDEADBEEFu);
    std::vector<uint8_t> ra(n), rb(has_b ? n : 0), writes(n * Dh, 0);
    if (!rd(f, obs.data(), obs.size()) || !rd(f, prev.data(), prev.size()) || !rd(f, ra.data(), ra.size()) || !rd(f, rb.data(), rb.size()))
        return 4;
    fclose(f);
    ObsHistArgs a{};
    a.obs = obs.data();
    a.prev = has_prev ? prev.data() : nullptr;
    a.reset_a = ra.data();
    a.reset_b = has_b ? rb.data() : nullptr;
    a.obs_stride = stride;
    a.n = (int32_t)n;
    a.Dh = (int32_t)Dh;
    a.n_terms = (int32_t)n_terms;
    a.shift = (int32_t)shift;
    a.total = (int32_t)(n * Dh);
    a.slots = (a.total + a.shift + OBSHIST_SLOT - 1) / OBSHIST_SLOT;
    int64_t whole = 0;
    for (int slot = 0; slot < a.slots; ++slot) {
        uint32_t v[OBSHIST_SLOT];
        int j0 = 0;
        const int count = obshist_gather(slot, a, t.data(), v, j0);
        if (count == OBSHIST_SLOT) {
            if ((j0 + a.shift) % OBSHIST_SLOT != 0) return 7;      // a whole slot must lie on a 16-byte line
            ++whole;
        }
        for (int i = 0; i < count; ++i) {
            next.at(j0 + i) = v[i];
            ++writes.at(j0 + i);
        }
    }
    const bool ok = wr(g, &Dh, 1) && wr(g, next.data(), next.size()) && wr(g, writes.data(), writes.size()) && wr(g, &whole, 1);
    return fclose(g) == 0 && ok ? 0 : 6;
}
