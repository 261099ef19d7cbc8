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
#define EPOCH_PROLOGUE
#define EPOCH_2D_ROW(r)
#define EPOCH_2D_TERM(dist) dist
#include "eval_epoch_body.inc"
#undef EPOCH_PROLOGUE
#undef EPOCH_2D_ROW
#undef EPOCH_2D_TERM
}

constexpr int kCountSlots = 1024;   // samples whose present-view count is kept in LDS; a sample beyond them has its mask row counted when asked

// Present views of one sample: its row of the view mask, counted.
__device__ __forceinline__ int count_views(const uint8_t *__restrict__ row, int V) {
    int n = 0;
    for (int v = 0; v < V; ++v) n += row[v] != 0;
    return n;
}

// One step of a ragged view set (present: [B][V], non-zero = the view is there).  Everything but the 2D sum is the uniform kernel's.
// The 2D rows are walked in its order; a present row of sample b adds its distance times V / v_b (exactly 1.0 for a full sample, so
// a full mask gives the uniform kernel's bits), an absent row is not read, and [5] still grows by B * V * 21: [6] / [5] stays the mean
// over samples of each sample's own 2D MPJPE over its present views.  A sample without a present view (a broken precondition) adds
// 0 * inf = NaN to [6]; nothing is indexed by a count.
__global__ __launch_bounds__(kThreads) void eval_epoch_views_kernel(EpochParams a, const uint8_t *__restrict__ present) {
    __shared__ int cnt[kCountSlots];
#define EPOCH_PROLOGUE \
    for (int b = t; b < a.B && b < kCountSlots; b += kThreads) cnt[b] = count_views(present + (long)b * a.V, a.V);
#define EPOCH_2D_ROW(r)                                                                                                             \
    const long slot = (r) / NJ, smp = slot / a.V;                                                                                   \
    const double wgt = (double)a.V / (double)(smp < kCountSlots ? cnt[smp] : count_views(present + smp * a.V, a.V));                \
    if (!present[slot]) {                                                                                                           \
        acc += 0.0 * wgt;                                                                                                           \
        continue;                                                                                                                   \
    }
#define EPOCH_2D_TERM(dist) (dist) * wgt
#include "eval_epoch_body.inc"
#undef EPOCH_PROLOGUE
#undef EPOCH_2D_ROW
#undef EPOCH_2D_TERM
}

int bad_arg(const char *who, const char *what) {
    hmv::set_thread_error(std::string(who) + ": " + what);
    return HMV_ERR_ARG;
}

int hip_fail(const char *who, hipError_t e) {
    hmv::set_thread_error(std::string(who) + ": " + hipGetErrorString(e));
    return HMV_ERR_HIP;
}

// the argument rules of the two entries, in front of every HIP call; 0 or the HMV_ERR_ARG of the first broken one
int check_eval_args(const char *who, const hmv_eval_args *a) {
    if (!a) return bad_arg(who, "args is NULL");
    if (a->struct_size != (int32_t)sizeof(hmv_eval_args)) return bad_arg(who, "struct_size does not match this library's hmv_eval_args");
    if (a->B < 1) return bad_arg(who, "B must be >= 1");
    if (a->V < 1) return bad_arg(who, "V must be >= 1");
    if ((int64_t)a->B * a->V > (1 << 24)) return bad_arg(who, "B * V must not exceed 2^24 frames");
    if (a->steps < 1 || a->steps > kMaxSteps) return bad_arg(who, "steps must be in 1 .. 256");
    if (!(a->thr_max >= a->thr_min)) return bad_arg(who, "thr_max must not be below thr_min");
    if (!a->pred_joints_cam) return bad_arg(who, "pred_joints_cam is NULL");
    if (!a->gt_joints_cam) return bad_arg(who, "gt_joints_cam is NULL");
    if (!a->pred_joints_2d) return bad_arg(who, "pred_joints_2d is NULL");
    if (!a->gt_joints_2d) return bad_arg(who, "gt_joints_2d is NULL");
    if (!a->state || ((uintptr_t)a->state & 7)) return bad_arg(who, "state is NULL or not 8-byte aligned");
    if (a->state_doubles < hmv_eval_state_doubles(a->steps))
        return bad_arg(who, "state_doubles is smaller than hmv_eval_state_doubles gives for steps");
    return HMV_OK;
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
    if (const int rc = check_eval_args(who, a)) return rc;
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    hipLaunchKernelGGL(eval_epoch_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, epoch_params(a));
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}

extern "C" int hmv_eval_add_views(int32_t device, const hmv_eval_args *a, const uint8_t *view_present, void *stream) {
    const char *who = "hmv_eval_add_views";
    if (const int rc = check_eval_args(who, a)) return rc;
    if (!view_present) return bad_arg(who, "view_present is NULL (hmv_eval_add is the entry for a batch with every view)");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    hipLaunchKernelGGL(eval_epoch_views_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, epoch_params(a), view_present);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}

extern "C" size_t hmv_eval_state_doubles(int32_t steps) {
    return steps >= 1 && steps <= kMaxSteps ? (size_t)(kScalars + 1 + steps) : 0;
}
