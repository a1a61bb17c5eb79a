// wl_obs_history_dev.h -- the index map of the observation-history push (see wl_obs_history.hip): which column of the raw row or of the
// previous stacked row every output of the new stacked row is a copy of.  __host__ __device__ and a header of its own so that
// tests/host_sim can run the same integer arithmetic on the host and hold it against the reference.  Nothing here is floating point:
// the values travel as 32-bit words.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/wheeledlab_amd_history.h"
#include "wl_layer_common.h"

namespace {

constexpr int OBSHIST_SLOT = 4;   // outputs per lane: one 16-byte store

// what a launch needs besides the table; `shift` = (address of next / 4) & 3, so that output j lies on a 16-byte boundary when
// (j + shift) % 4 == 0, and slot s holds the outputs [4 s - shift, 4 s - shift + 4) that exist
struct ObsHistArgs {
    const uint32_t* obs;
    const uint32_t* prev;       // NULL: every row is filled from its raw row
    const uint8_t* reset_a;
    const uint8_t* reset_b;     // may be NULL
    int64_t obs_stride;
    int32_t n, Dh, n_terms, shift;
    int32_t total;              // n * Dh < 2^31 - 16
    int32_t slots;              // (total + shift + 3) / 4
};

// the validated table: term k covers columns [dst_off, dst_off + width * frames) of the stacked row, in order, without gaps
WL_HD int64_t obshist_width(const WlObsHistoryTerm* t, int n_terms, int D) {
    if (!t || n_terms < 1 || n_terms > WL_OBSHIST_MAX_TERMS || D < 1 || D > WL_OBSHIST_MAX_DIM) return -1;
    int64_t src = 0, dst = 0;
    for (int k = 0; k < n_terms; ++k) {
        if (t[k].width < 1 || t[k].width > D || t[k].frames < 1 || t[k].frames > WL_OBSHIST_MAX_FRAMES) return -1;
        if (t[k].src_off != src || t[k].dst_off != dst) return -1;
        src += t[k].width;
        dst += (int64_t)t[k].width * t[k].frames;
    }
    return src == D ? dst : -1;
}

// a position in the stacked row: column c = dst_off_k + r, r = frame * width + column inside the frame
struct ObsHistCursor {
    int32_t k, r;
    int32_t src_off, w, span;   // of term k; span = w * frames
};

WL_HD void obshist_load_term(ObsHistCursor& q, const WlObsHistoryTerm* t) {
    q.src_off = t[q.k].src_off;
    q.w = t[q.k].width;
    q.span = t[q.k].width * t[q.k].frames;
}

// the term of column c: the last k with dst_off_k <= c, six halvings over at most 64 entries
WL_HD ObsHistCursor obshist_seek(int c, const WlObsHistoryTerm* t, int n_terms) {
    int k = 0;
#pragma unroll
    for (int step = WL_OBSHIST_MAX_TERMS / 2; step > 0; step >>= 1) {
        const int m = k + step;
        if (m < n_terms && t[m].dst_off <= c) k = m;
    }
    ObsHistCursor q;
    q.k = k;
    q.r = c - t[k].dst_off;
    obshist_load_term(q, t);
    return q;
}

// to the next column of the row; true: that was the row's last column and the cursor stands on column 0 of the next row
WL_HD bool obshist_step(ObsHistCursor& q, const WlObsHistoryTerm* t, int n_terms) {
    if (++q.r < q.span) return false;
    const bool wrapped = q.k + 1 == n_terms;
    q.k = wrapped ? 0 : q.k + 1;
    q.r = 0;
    obshist_load_term(q, t);
    return wrapped;
}

// Column c (where the cursor stands) of a stacked row is a copy of: column `col` of the env's raw row (from_obs), or column `col` of
// its previous stacked row.  The newest frame is the raw row's slice; an older frame f of a running env is frame f + 1 of the
// previous row, w columns further on; of a fresh env (reset, or no previous row) every frame is the raw row's slice.
struct ObsHistSrc {
    int32_t col;
    bool from_obs;
};
WL_HD ObsHistSrc obshist_source(const ObsHistCursor& q, int c, bool fresh) {
    const int newest = q.span - q.w;
    if (q.r >= newest) return ObsHistSrc{q.src_off + (q.r - newest), true};
    if (fresh) return ObsHistSrc{q.src_off + (int)((unsigned)q.r % (unsigned)q.w), true};
    return ObsHistSrc{c + q.w, false};
}

WL_HD bool obshist_fresh(const ObsHistArgs& a, int e) {
    return !a.prev || WL_LAYER_RESET(a, e);
}

// the outputs of slot s: v[0 .. count) are outputs j0 .. j0 + count - 1 of the flat [n][Dh] block; count == 4 exactly when the slot
// is a whole 16-byte line of `next`
WL_HD int obshist_gather(int slot, const ObsHistArgs& a, const WlObsHistoryTerm* t, uint32_t (&v)[OBSHIST_SLOT], int& j0) {
    const int v0 = slot * OBSHIST_SLOT - a.shift;
    j0 = v0 < 0 ? 0 : v0;
    const int j1 = v0 + OBSHIST_SLOT < a.total ? v0 + OBSHIST_SLOT : a.total;
    if (j1 <= j0) return 0;
    int e = (int)((unsigned)j0 / (unsigned)a.Dh);
    int c = j0 - e * a.Dh;
    ObsHistCursor q = obshist_seek(c, t, a.n_terms);
    bool fresh = obshist_fresh(a, e);
#pragma unroll
    for (int i = 0; i < OBSHIST_SLOT; ++i) {
        if (j0 + i >= j1) break;
        const ObsHistSrc s = obshist_source(q, c, fresh);
        const uint32_t* p = s.from_obs ? a.obs + (int64_t)e * a.obs_stride + s.col : a.prev + (int64_t)e * a.Dh + s.col;
        v[i] = *p;
        ++c;
        if (obshist_step(q, t, a.n_terms)) {
            c = 0;
            ++e;
            if (j0 + i + 1 < j1) fresh = obshist_fresh(a, e);
        }
    }
    return j1 - j0;
}

}  // namespace
