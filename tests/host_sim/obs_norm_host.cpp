// TEST INFRASTRUCTURE ONLY: the observation normaliser's arithmetic (wheeledlab_amd/csrc/wl_obs_norm_dev.h: one element's moments,
// the merge into the running state, the folded first layer, the launch plan) compiled for the host through the stand-in
// hip_runtime.h, as a stand-alone program that tests/test_obs_norm_host_cpu.py holds against the float64 reference without a GPU --
// and the place for -fsanitize=address,undefined runs of that code.
//
//   obs_norm_host IN OUT
// IN : int64 rows, D, H, row_stride, count, until, merges; double eps; float mean[D], var[D], x[rows][row_stride], w1[H][D], b1[H]
// OUT: double sums[2][D] (of the LAST merge); float mean[D], var[D], std[D], inv_std[D]; int64 count; float out[rows][row_stride]
//      (x normalised with the statistics before the last merge); float w1_out[H][D], b1_out[H] (folded with the final statistics);
//      int64 narrow, partials, per_partial (the launch plan of this shape)
// `merges` > 1 cuts the rows into that many equal batches merged one after the other (rows % merges == 0).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

#include "wl_obs_norm_dev.h"

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
    double eps;
    if (!rd(f, h, 7) || !rd(f, &eps, 1)) return 4;
    const int64_t rows = h[0], D = h[1], H = h[2], stride = h[3], until = h[5], merges = h[6];
    int64_t count = h[4];
    if (rows < 1 || D < 1 || H < 1 || stride < D || merges < 1 || rows % merges) return 5;
    std::vector<float> mean(D), var(D), sd(D), inv(D), x(rows * stride), w1(H * D), b1(H);
    if (!rd(f, mean.data(), D) || !rd(f, var.data(), D) || !rd(f, x.data(), x.size()) || !rd(f, w1.data(), w1.size()) || !rd(f, b1.data(), H))
        return 4;
    fclose(f);
    for (int64_t c = 0; c < D; ++c) {
        sd[c] = (float)sqrt((double)var[c]);
        inv[c] = (float)(1.0 / (sqrt((double)var[c]) + eps));
    }
    std::vector<double> sums(2 * D);
    std::vector<float> out(x.size(), 0.f);
    const int64_t m = rows / merges;
    for (int64_t k = 0; k < merges; ++k) {
        for (int64_t c = 0; c < D; ++c) {
            double s1 = 0.0, s2 = 0.0;
            for (int64_t r = k * m; r < (k + 1) * m; ++r) {
                obsnorm_add(x[r * stride + c], mean[c], s1, s2);
                if (k == merges - 1) out[r * stride + c] = obsnorm_apply(x[r * stride + c], mean[c], inv[c]);
            }
            sums[c] = s1;
            sums[D + c] = s2;
        }
        if (count >= until) continue;
        count += m;
        for (int64_t c = 0; c < D; ++c) {
            const ObsNormState s = obsnorm_merge(sums[c], sums[D + c], (double)m, (double)count, mean[c], var[c], eps);
            mean[c] = s.mean, var[c] = s.var, sd[c] = s.std, inv[c] = s.inv_std;
        }
    }
    std::vector<float> w1o(H * D), b1o(H);
    for (int64_t j = 0; j < H; ++j) {
        double s = 0.0;
        for (int64_t c = 0; c < D; ++c) {
            w1o[j * D + c] = obsnorm_fold_weight(w1[j * D + c], inv[c]);
            s += obsnorm_fold_term(w1[j * D + c], mean[c], inv[c]);
        }
        b1o[j] = (float)((double)b1[j] - s);
    }
    const ObsNormPlan p = obsnorm_plan(rows, (int)D, stride);
    const int64_t plan[3] = {p.narrow, p.partials, p.per_partial};
    f = fopen(argv[2], "wb");
    if (!f) return 3;
    const bool ok = wr(f, sums.data(), sums.size()) && wr(f, mean.data(), D) && wr(f, var.data(), D) && wr(f, sd.data(), D) &&
                    wr(f, inv.data(), D) && wr(f, &count, 1) && wr(f, out.data(), out.size()) && wr(f, w1o.data(), w1o.size()) &&
                    wr(f, b1o.data(), H) && wr(f, plan, 3);
    return fclose(f) == 0 && ok ? 0 : 6;
}
