// An evaluation epoch on the device: per step one launch adds what HandMvNet._calculate_mpjpe (handmvnet.py:370-427) computes -- and the
// loss vector hmv_pose_losses wrote -- into a caller-owned fp64 state vector (layout: include/handmv.h), so that a whole split is read
// back once.  The epoch value of every quantity is sum(B * step value) / sum(B).
//
// Shaped like pose_metrics_kernel and built from the same device functions (pose_rows.h): one workgroup, fixed-order LDS tree
// reductions, no float atomics, fp32 for the distance-versus-threshold comparison, fp64 for sums and the 3x3 Procrustes problem.
// The state is read and written by one thread at the end of the kernel in plain C++; stream order orders successive steps.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/handmv.h"
#include "kernels.h"
#include "pose_rows.h"

namespace {

constexpr int NJ = 21;
constexpr int kScalars = 14;   // state[0 .. 14): counts and sums; the histogram follows

struct EpochParams {
    const float *pred_cam, *gt_cam, *pred_2d, *gt_2d, *loss;
    const uint8_t *mask;
    double *state;
    int B, V, steps, n_pts;
    float tmin, tmax;
};

__global__ __launch_bounds__(kThreads) void eval_epoch_kernel(EpochParams a) {
    __shared__ double red[kThreads];
    __shared__ float thr[kMaxSteps];
    __shared__ int hist[kMaxSteps + 1];
    const int t = threadIdx.x;
    fill_thresholds(thr, a.tmin, a.tmax, a.steps);
    if (t <= a.steps) hist[t] = 0;
    __syncthreads();

    // ---- the 3D distances that remain after the similarity alignment of each pose, one lane per pose.  First, while nothing else
    // is live: the alignment needs every register a lane has
    double acc = 0.0;
    for (int first = 0; first < a.B; first += kThreads) {   // a uniform counter: the lane keeps no loop state of its own
        const int sidx = first + t;
        if (sidx >= a.B) continue;
        const float *p = a.pred_cam + (long)sidx * NJ * 3;
        const float *g = a.gt_cam + (long)sidx * NJ * 3;
        float *const no_output = nullptr;
        double U[3][3], S[3], V[3][3];
        {
            POSE_MOMENTS(p, g, a.n_pts, mu1, mu2, var1, K)
            svd3(K, U, S, V);
            (void)var1;
        }
        // the moments again rather than kept: with them live across svd3 the lane's working set does not fit the 128 registers a
        // 1024-lane workgroup leaves it
        POSE_MOMENTS(p, g, a.n_pts, mu1, mu2, var1, K)
        POSE_ADD_ALIGNED_ERROR(p, g, a.n_pts, mu1, mu2, var1, K, U, V, no_output, 0L, acc)
    }
    const double sum_pa = block_sum(acc, red);

    // ---- 3D: joint distances and their PCK bins
    const long rows3 = (long)a.B * NJ;
    acc = 0.0;
    for (long r = t; r < rows3; r += kThreads) {
        const float dist = row_distance(a.pred_cam + r * 3, a.gt_cam + r * 3, 3);
        acc += (double)dist;
        atomicAdd(&hist[threshold_bin(dist, thr, a.steps)], 1);
    }
    const double sum3 = block_sum(acc, red);

    // ---- 2D: masked joints are zeroed on both sides (models/utils.py:123-131), so they add 0 and still count
    const long rows2 = (long)a.B * a.V * NJ;
    acc = 0.0;
    for (long r = t; r < rows2; r += kThreads) {
        const float keep = (a.mask && a.mask[r]) ? 0.f : 1.f;
        const float p[2] = {a.pred_2d[r * 2] * keep, a.pred_2d[r * 2 + 1] * keep};
        const float g[2] = {a.gt_2d[r * 2] * keep, a.gt_2d[r * 2 + 1] * keep};
        acc += (double)row_distance(p, g, 2);
    }
    const double sum2 = block_sum(acc, red);   // its leading barrier also completes hist

    if (t == 0) {
        double *s = a.state;
        s[0] += (double)a.B;
        s[1] += 1.0;
        s[2] += (double)rows3;
        s[3] += sum3;
        s[4] += sum_pa;
        s[5] += (double)rows2;
        s[6] += sum2;
        if (a.loss) {
            s[7] += (double)a.B;
            for (int i = 0; i < 6; ++i) s[8 + i] += (double)a.B * (double)a.loss[i];
        }
        for (int i = 0; i <= a.steps; ++i) s[kScalars + i] += (double)hist[i];
    }
}

int bad_arg(const char *what) {
    hmv::set_thread_error(std::string("hmv_eval_add: ") + what);
    return HMV_ERR_ARG;
}

int hip_fail(hipError_t e) {
    hmv::set_thread_error(std::string("hmv_eval_add: ") + hipGetErrorString(e));
    return HMV_ERR_HIP;
}

}  // namespace

extern "C" size_t hmv_eval_state_doubles(int32_t steps) {
    return steps >= 1 && steps <= kMaxSteps ? (size_t)(kScalars + 1 + steps) : 0;
}

extern "C" int hmv_eval_add(int32_t device, const hmv_eval_args *a, void *stream) {
    if (!a) return bad_arg("args is NULL");
    if (a->struct_size != (int32_t)sizeof(hmv_eval_args)) return bad_arg("struct_size does not match this library's hmv_eval_args");
    if (a->B < 1) return bad_arg("B must be >= 1");
    if (a->V < 1) return bad_arg("V must be >= 1");
    if ((int64_t)a->B * a->V > (1 << 24)) return bad_arg("B * V must not exceed 2^24 frames");
    if (a->steps < 1 || a->steps > kMaxSteps) return bad_arg("steps must be in 1 .. 256");
    if (!(a->thr_max >= a->thr_min)) return bad_arg("thr_max must not be below thr_min");
    if (!a->pred_joints_cam) return bad_arg("pred_joints_cam is NULL");
    if (!a->gt_joints_cam) return bad_arg("gt_joints_cam is NULL");
    if (!a->pred_joints_2d) return bad_arg("pred_joints_2d is NULL");
    if (!a->gt_joints_2d) return bad_arg("gt_joints_2d is NULL");
    if (!a->state || ((uintptr_t)a->state & 7)) return bad_arg("state is NULL or not 8-byte aligned");
    if (a->state_doubles < hmv_eval_state_doubles(a->steps))
        return bad_arg("state_doubles is smaller than hmv_eval_state_doubles gives for steps");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(hipGetLastError());
    EpochParams k;
    k.pred_cam = a->pred_joints_cam; k.gt_cam = a->gt_joints_cam; k.pred_2d = a->pred_joints_2d; k.gt_2d = a->gt_joints_2d;
    k.loss = a->loss_result; k.mask = a->joints_mask; k.state = a->state;
    k.B = a->B; k.V = a->V; k.steps = a->steps; k.n_pts = NJ;
    k.tmin = a->thr_min; k.tmax = a->thr_max;
    hipLaunchKernelGGL(eval_epoch_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, k);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(e);
}
