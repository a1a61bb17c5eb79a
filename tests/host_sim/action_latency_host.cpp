// TEST INFRASTRUCTURE ONLY: the per-env bodies of the action-latency layer (wheeledlab_amd/csrc/wl_action_latency_dev.h: the push into the
// ring, the delayed read, the reset's lag draw, the policy's action back into the state rows and the observation columns) compiled for
// the host through the stand-in hip_runtime.h, as a stand-alone program that tests/test_action_latency_cpu.py holds against the
// reference without a GPU -- and the place for -fsanitize=address,undefined runs of that code.  Every buffer is allocated at its exact
// size, so an index the bodies get wrong is an out-of-bounds access the sanitizer reports.
//
//   action_latency_host IN OUT        the case file in, the results out
//   action_latency_host --med3        prints the words of the stand-in's median of (x, -1, 1) for x a signalling and a quiet NaN
// IN : int64 n, stride, min_delay, max_delay, per_component, clip_wrapper, row_pitch, col, has_reset_b, ops; uint64 seed, env_offset;
//      uint32 state[WL_S_COUNT][stride]; uint32 row[n][row_pitch] (if col >= 0); uint32 block[rows][stride]; then per operation:
//      int64 kind (0 push, 1 finish); uint32 action[n][2]; finish only: uint8 reset_a[n]; uint8 reset_b[n] (if has_reset_b)
// OUT: int64 rows (or -1 and nothing else: max_delay was refused); after every operation: uint32 applied[n][2]; uint32
//      state[WL_S_COUNT][stride]; uint32 row[n][row_pitch] (if col >= 0); uint32 block[rows][stride]
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "wl_action_latency_dev.h"

namespace {
template <class T>
bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
template <class T>
bool wr(FILE* f, const T* p, size_t n) { return n == 0 || fwrite(p, sizeof(T), n, f) == n; }
}  // namespace

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "--med3") == 0) {
        const uint32_t in[2] = {0x7F800001u, 0x7FC00001u};
        for (uint32_t w : in) {
            volatile float x;
            std::memcpy((void*)&x, &w, 4);
            const float y = clampf(x, -1.f, 1.f);
            uint32_t o;
            std::memcpy(&o, &y, 4);
            std::printf("%u ", o);
        }
        return 0;
    }
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 3;
    int64_t h[10];
    uint64_t key[2];
    if (!rd(f, h, 10) || !rd(f, key, 2)) return 4;
    const int64_t n = h[0], stride = h[1], lo = h[2], hi = h[3], per = h[4], clip = h[5], pitch = h[6], col = h[7], has_b = h[8], ops = h[9];
    if (n < 1 || stride < n || ops < 0 || pitch < 1 || col < -1 || col > pitch - 2 || lo < 0 || lo > hi) return 5;
    const int64_t rows = actlat_width((int)(hi > 1024 ? 1024 : hi));
    FILE* g = fopen(argv[2], "wb");
    if (!g) return 3;
    if (rows < 0) {
        const int64_t bad = -1;
        const bool ok = wr(g, &bad, 1);
        return fclose(g) == 0 && ok ? 0 : 6;
    }
    std::vector<float> state(WL_S_COUNT * stride), row(col >= 0 ? n * pitch : 0), action(2 * n);      // (words: read and written as they are)
    std::vector<uint32_t> block(rows * stride), applied(2 * n, 0u);
    std::vector<uint8_t> ra(n), rb(has_b ? n : 0);
    if (!rd(f, state.data(), state.size()) || !rd(f, row.data(), row.size()) || !rd(f, block.data(), block.size())) return 4;
    bool ok = wr(g, &rows, 1);
    for (int64_t c = 0; c < ops; ++c) {
        int64_t kind;
        if (!rd(f, &kind, 1) || !rd(f, action.data(), action.size())) return 4;
        if (kind == 0) {
            ActLatPushArgs a{};
            a.action = reinterpret_cast<const uint32_t*>(action.data());
            a.applied = applied.data();
            a.block = block.data();
            a.stride = stride;
            a.n = (int32_t)n;
            a.max_delay = (int32_t)hi;
            for (int e = 0; e < a.n; ++e) actlat_push_env(e, a);
        } else {
            if (!rd(f, ra.data(), ra.size()) || !rd(f, rb.data(), rb.size())) return 4;
            ActLatFinishArgs a{};
            a.action = action.data();
            a.state = state.data();
            a.row = col >= 0 ? row.data() : nullptr;
            a.block = block.data();
            a.reset_a = ra.data();
            a.reset_b = has_b ? rb.data() : nullptr;
            a.stride = stride;
            a.row_pitch = pitch;
            a.seed = key[0];
            a.env0 = (uint32_t)key[1];
            a.n = (int32_t)n;
            a.col = (int32_t)col;
            a.min_delay = (int32_t)lo;
            a.max_delay = (int32_t)hi;
            a.per_component = (int32_t)per;
            a.clip_wrapper = (int32_t)clip;
            for (int e = 0; e < a.n; ++e) actlat_finish_env(e, a);
        }
        ok = ok && wr(g, applied.data(), applied.size()) && wr(g, state.data(), state.size()) && wr(g, row.data(), row.size()) &&
             wr(g, block.data(), block.size());
    }
    fclose(f);
    return fclose(g) == 0 && ok ? 0 : 6;
}
