// wl_layer_common.h -- what the four between-step layers share (wl_obs_history, wl_obs_corrupt, wl_event_rand, wl_action_latency: each a
// .hip with its entry points and a _dev.h with its per-env body).  It compiles for the host through the stand-in
// hip_runtime.h of tests/host_sim, where the span check is tested on its own (tests/host_sim/layer_spans_host.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

#define WL_HD __host__ __device__ __forceinline__   // integer / table code the host entry points call too

// Env e of the argument block `a` was reset by the step: either flag row says so (a.reset_b may be NULL).  A macro: as an inline function
// (the pointers by value or by reference, or the block) it moved the argument loads of the event and the latency `finish` kernel above
// their bounds test and changed both kernels' code; as text, all four compile to what they were.  UNSAFE with side effects: `a` and `e`
// are evaluated more than once.
#define WL_LAYER_RESET(a, e) (((a).reset_a[e] | ((a).reset_b ? (a).reset_b[e] : (uint8_t)0)) != 0)

WL_HD bool layer_finite(float x) { return x - x == 0.f; }

#ifndef WL_HOST_SIM
// a table that arrived by value with the launch (nothing is staged, so the call can be captured) into the workgroup's LDS copy `t`, where
// the term loops index it; every thread of the block calls it, before any leaves
template <class Term, int N, class Table>
__device__ __forceinline__ void layer_table_to_lds(Term (&t)[N], const Table& tab, int n_terms) {
    if ((int)threadIdx.x < n_terms) t[threadIdx.x] = tab.t[threadIdx.x];
    __syncthreads();
}
#endif

// ---- host: what a launch stores may touch nothing else it reads or stores
inline bool overlap(const void* p, int64_t p_bytes, const void* q, int64_t q_bytes) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + (uintptr_t)q_bytes && b < a + (uintptr_t)p_bytes;
}

struct Span {   // one buffer argument of an entry point: the bytes the launch may touch from p on; p NULL: an optional argument, absent
    const void* p;
    int64_t bytes;
};

// Does one of the first `stored` spans, which the launch writes, lie on any other span?  Spans that touch end to start do not overlap, a
// NULL span overlaps nothing, and two spans the launch only reads may lie on each other.
template <int N>
bool any_overlap(const Span (&v)[N], int stored) {
    for (int i = 0; i < stored; ++i)
        for (int j = i + 1; j < N; ++j)
            if (v[i].p && v[j].p && overlap(v[i].p, v[i].bytes, v[j].p, v[j].bytes)) return true;
    return false;
}

}  // namespace
