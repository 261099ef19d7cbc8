// Evaluation metrics on the device: MPJPE, Procrustes-aligned MPJPE and the PCK curve / AUC the
// reference logs from test_step (handmvnet.py:352-368 -> models/metrics.py:6-24, 64-123, 128-176).
//
// The inputs are tiny ([b,21,3] per step), so this is one single-workgroup launch: deterministic
// block-level reductions (fixed-order LDS tree, no float atomics), one lane per pose for the 3x3
// Procrustes problem.  The arithmetic that decides a comparison (joint distance vs threshold) is fp32 like
// the reference's; sums and the 3x3 SVD run in fp64.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/handmv.h"
#include "pose_rows.h"

namespace {

constexpr int kThreads = 1024;   // the one workgroup of the launch

// result: [0] mean distance, [1] mean distance after similarity alignment (NaN when not requested),
//         [2] auc, [3] norm_auc, [4 .. 4+steps) pck values, [4+steps .. 4+2*steps) thresholds.
__global__ __launch_bounds__(kThreads) void pose_metrics_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                               int n_sets, int n_pts, int dim, float tmin, float tmax,
                                                               int steps, int procrustes, float* __restrict__ aligned,
                                                               float* __restrict__ result) {
    __shared__ double red[kThreads];
    __shared__ float thr[kMaxSteps];
    __shared__ int hist[kMaxSteps + 1];
    const int t = threadIdx.x;
    fill_thresholds(thr, tmin, tmax, steps);
    if (t <= steps) hist[t] = 0;
    __syncthreads();

    // ---- MPJPE (metrics.py:12) and the PCK histogram (metrics.py:77-85)
    const long rows = (long)n_sets * n_pts;
    double dsum = 0.0;
    for (long r = t; r < rows; r += kThreads) {
        const float dist = distance_n(pred + r * dim, gt + r * dim, dim);
        dsum += (double)dist;
        atomicAdd(&hist[threshold_bin(dist, thr, steps)], 1);
    }
    const double mean_dist = block_sum<kThreads>(dsum, red) / (double)rows;

    // ---- PA-MPJPE: similarity transform of each predicted pose onto its target (metrics.py:128-176)
    double pasum = 0.0;
    if (procrustes) {
        for (int sidx = t; sidx < n_sets; sidx += kThreads) {
            const float* p = pred + (long)sidx * n_pts * 3;
            const float* g = gt + (long)sidx * n_pts * 3;
            PoseMoments m;
            pose_moments(p, g, n_pts, m);
            double U[3][3], S[3], V[3][3];
            svd3(m.K, U, S, V);
            float* out = aligned ? aligned + (long)sidx * n_pts * 3 : nullptr;
            pose_aligned_points(p, g, n_pts, m, U, V, [&](int j, const double* y, double dist) {
                if (out)
                    for (int c = 0; c < 3; ++c) out[j * 3 + c] = (float)y[c];
                pasum += dist;
            });
        }
    }
    const double pa_mean = block_sum<kThreads>(pasum, red) / (double)rows;

    if (t == 0) {
        result[0] = (float)mean_dist;
        result[1] = procrustes ? (float)pa_mean : nanf("");
        // PCK curve: cumulative histogram; AUC by the trapezoidal rule in fp32 (metrics.py:114-121)
        int cum = 0;
        float auc = 0.f, one = 0.f, prev = 0.f;
        for (int i = 0; i < steps; ++i) {
            cum += hist[i];
            const float pck = (float)cum / (float)rows;
            result[4 + i] = pck;
            result[4 + steps + i] = thr[i];
            if (i > 0) {
                const float dx = thr[i] - thr[i - 1];
                auc += dx * (pck + prev) * 0.5f;
                one += dx;
            }
            prev = pck;
        }
        result[2] = auc;
        result[3] = auc / one;   // 0/0 = NaN for a single threshold, like the reference
    }
}

}  // namespace

extern "C" int hmv_pose_metrics(int32_t device, const float* pred, const float* target, int32_t n_sets, int32_t n_pts,
                                int32_t dim, float thr_min, float thr_max, int32_t steps, int32_t procrustes,
                                float* aligned, float* result, void* stream) {
    if (!pred || !target || !result || n_sets <= 0 || n_pts <= 0 || dim < 1 || dim > 4 || steps < 1 || steps > kMaxSteps)
        return HMV_ERR_ARG;
    if ((procrustes || aligned) && dim != 3) return HMV_ERR_ARG;
    if (aligned && !procrustes) return HMV_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return HMV_ERR_HIP;
    hipLaunchKernelGGL(pose_metrics_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, pred, target, n_sets, n_pts, dim,
                       thr_min, thr_max, steps, procrustes, aligned, result);
    return hipGetLastError() == hipSuccess ? HMV_OK : HMV_ERR_HIP;
}
