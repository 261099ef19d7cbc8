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

#include "../../include/handmv.h"
#include "kernels.h"
#include "pose_rows.h"

namespace {

constexpr int kThreads = 1024;   // the one workgroup of the launch
constexpr int kScalars = 14;     // state[0 .. 14): counts and sums; the histogram follows
static_assert(kMaxSteps == hmv::kMaxEvalSteps, "check_eval_args refuses what the kernels' LDS tables cannot hold");

struct EpochParams {
    const float *pred_cam, *gt_cam, *pred_2d, *gt_2d, *loss;
    const uint8_t *mask;
    double *state;
    int B, V, steps, n_pts;
    float tmin, tmax;
};

// One step, by the one workgroup.  kRagged: a ragged view set (present: [B][V], non-zero = the view is there; cnt: kCountSlots ints
// of LDS).  Everything but the 2D sum is the uniform step's.  The 2D rows are walked in its order; a present row of sample b adds its
// distance times V / v_b (exactly 1.0 for a full sample, so a full mask gives the uniform kernel's bits), an absent row is not read,
// and [5] still grows by B * V * 21: [6] / [5] stays the mean over samples of each sample's own 2D MPJPE over its present views.  A
// sample without a present view (a broken precondition) adds 0 * inf = NaN to [6]; nothing is indexed by a count.
template <bool kRagged>
__device__ __forceinline__ void epoch_step(const EpochParams &a, const uint8_t *__restrict__ present, int *cnt) {
    __shared__ double red[kThreads];
    __shared__ float thr[kMaxSteps];
    __shared__ int hist[kMaxSteps + 1];
    const int t = threadIdx.x;
    if constexpr (kRagged) fill_view_counts<kThreads>(cnt, present, a.B, a.V);
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
        double U[3][3], S[3], V[3][3];
        PoseMoments m;
        pose_moments(p, g, a.n_pts, m);
        svd3(m.K, U, S, V);
        // the moments again rather than kept: with them live across svd3 the lane's working set does not fit the 128 registers a
        // 1024-lane workgroup leaves it
        pose_moments(p, g, a.n_pts, m);
        pose_aligned_points(p, g, a.n_pts, m, U, V, [&](int, const double *, double dist) { acc += dist; });
    }
    const double sum_pa = block_sum<kThreads>(acc, red);

    // ---- 3D: joint distances and their PCK bins
    const long rows3 = (long)a.B * NJ;
    acc = 0.0;
    for (long r = t; r < rows3; r += kThreads) {
        const float dist = distance_3(a.pred_cam + r * 3, a.gt_cam + r * 3);
        acc += (double)dist;
        atomicAdd(&hist[threshold_bin(dist, thr, a.steps)], 1);
    }
    const double sum3 = block_sum<kThreads>(acc, red);

    // ---- 2D: masked joints are zeroed on both sides (models/utils.py:123-131), so they add 0 and still count
    const long rows2 = (long)a.B * a.V * NJ;
    acc = 0.0;
    for (long r = t; r < rows2; r += kThreads) {
        double wgt = 1.0;
        if constexpr (kRagged) {
            const long slot = r / NJ;
            wgt = view_weight(present, cnt, slot / a.V, a.V);
            if (!present[slot]) {
                acc += 0.0 * wgt;
                continue;
            }
        }
        const float keep = (a.mask && a.mask[r]) ? 0.f : 1.f;
        const float p[2] = {a.pred_2d[r * 2] * keep, a.pred_2d[r * 2 + 1] * keep};
        const float g[2] = {a.gt_2d[r * 2] * keep, a.gt_2d[r * 2 + 1] * keep};
        const double dist = (double)distance_2(p, g);
        if constexpr (kRagged)
            acc += dist * wgt;
        else
            acc += dist;
    }
    const double sum2 = block_sum<kThreads>(acc, red);   // its leading barrier also completes hist

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

// Two kernels and not one with a nullable mask: the uniform one allocates no count array and tests no `present`, and it is the
// reference the tests hold the ragged one to under a full mask.
__global__ __launch_bounds__(kThreads) void eval_epoch_kernel(EpochParams a) { epoch_step<false>(a, nullptr, nullptr); }

__global__ __launch_bounds__(kThreads) void eval_epoch_views_kernel(EpochParams a, const uint8_t *__restrict__ present) {
    __shared__ int cnt[kCountSlots];
    epoch_step<true>(a, present, cnt);
}

using hmv::bad_arg;
using hmv::hip_fail;

int check_args(const char *who, const hmv_eval_args *a) {
    return hmv::check_eval_args(who, a, "hmv_eval_args", hmv_eval_state_doubles(a ? a->steps : 0),
                                "state_doubles is smaller than hmv_eval_state_doubles gives for steps");
}

EpochParams epoch_params(const hmv_eval_args *a) {
    EpochParams k;
    k.pred_cam = a->pred_joints_cam; k.gt_cam = a->gt_joints_cam; k.pred_2d = a->pred_joints_2d; k.gt_2d = a->gt_joints_2d;
    k.loss = a->loss_result; k.mask = a->joints_mask; k.state = a->state;
    k.B = a->B; k.V = a->V; k.steps = a->steps; k.n_pts = NJ;
    k.tmin = a->thr_min; k.tmax = a->thr_max;
    return k;
}

}  // namespace

extern "C" int hmv_eval_add(int32_t device, const hmv_eval_args *a, void *stream) {
    const char *who = "hmv_eval_add";
    if (const int rc = check_args(who, a)) return rc;
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    hipLaunchKernelGGL(eval_epoch_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, epoch_params(a));
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}

extern "C" int hmv_eval_add_views(int32_t device, const hmv_eval_args *a, const uint8_t *view_present, void *stream) {
    const char *who = "hmv_eval_add_views";
    if (const int rc = check_args(who, a)) return rc;
    if (!view_present) return bad_arg(who, "view_present is NULL (hmv_eval_add is the entry for a batch with every view)");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    hipLaunchKernelGGL(eval_epoch_views_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, epoch_params(a), view_present);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}

extern "C" size_t hmv_eval_state_doubles(int32_t steps) {
    return steps >= 1 && steps <= kMaxSteps ? (size_t)(kScalars + 1 + steps) : 0;
}
