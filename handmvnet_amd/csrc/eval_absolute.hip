// Absolute position over an evaluation epoch on the device: per step ONE launch adds what forward_absolute's triangulation says about
// the step -- the world MPJPE with the triangulated root, the root's own error, plain triangulation's error per joint, the status of
// every joint, the reprojection error per camera and the inlier histogram -- into a third caller-owned fp64 state (layout:
// include/handmv.h, "absolute evaluation").
//
// eval_epoch.hip's discipline: fp32 for a distance (distance_3 of pose_rows.h, on sums rounded to fp32 as the evaluation step makes
// them), fp64 for sums, every sum in a fixed order, no floating-point atomics.  A few workgroups, each the only writer of its slice of
// the state, each element read-modify-written by one lane in plain C++; stream order orders successive steps:
//   workgroup 0   the header, the located samples, [4], [5] and W
//   workgroup 1   T, TN and S
//   then          R and RN when reproj_err is given, H when inliers is given
// Samples are taken in chunks of kLanes; a chunk's per-row values are staged in LDS, lane j < 21 then adds column j down the chunk in
// sample order.  The kernel reports and repairs nothing: a non-finite distance of a located sample goes into the sums as it is.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/handmv.h"
#include "kernels.h"
#include "pose_rows.h"

namespace {

constexpr int kLanes = 256;       // lanes of a workgroup and samples of a staged chunk
constexpr int kMaxViews = 16;     // hmv_op_triangulate's
constexpr int kFixed = 155;       // state[0 .. 155): header (8), W, T, TN (21 each), S (84); then R[V], RN[V], H[V + 1]
constexpr int kW = 8, kT = kW + NJ, kTN = kT + NJ, kS = kTN + NJ;

struct AbsoluteParams {
    const float *pred_cam, *tri, *gt_cam, *gt_root, *reproj;
    const int32_t *status, *inliers;
    double *state;
    int B, V;
};

__device__ __forceinline__ bool finite_3(const float *p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

// a sample is located when its root joint was triangulated: status 0 and three finite coordinates
__device__ __forceinline__ bool located(const AbsoluteParams &a, long b) { return a.status[b * NJ] == 0 && finite_3(a.tri + b * NJ * 3); }

// out = x + y, each coordinate rounded to fp32 on its own: the evaluation step's joints_cam + root_joint
__device__ __forceinline__ void add_3(const float *x, const float *y, float *out) {
#pragma clang fp contract(off)
    out[0] = x[0] + y[0];
    out[1] = x[1] + y[1];
    out[2] = x[2] + y[2];
}

// ---- workgroup 0: the world distance per joint over the located samples, the root's error, the header
__device__ __forceinline__ void world(const AbsoluteParams &a) {
    __shared__ float dist[kLanes * NJ];
    __shared__ float root_dist[kLanes];
    __shared__ uint8_t found[kLanes];
    __shared__ double column[NJ];
    const int t = threadIdx.x;
    double col = 0.0, n_found = 0.0, root_sum = 0.0;   // lane j < 21: W[j];  lane 21: [3] and [5]
    for (int first = 0; first < a.B; first += kLanes) {
        const int n = min(kLanes, a.B - first);
        if (t < n) {
            const long b = first + t;
            const bool ok = located(a, b);
            found[t] = ok;
            root_dist[t] = ok ? distance_3(a.tri + b * NJ * 3, a.gt_root + b * 3) : 0.f;
        }
        for (int r = t; r < n * NJ; r += kLanes) {
            const long b = first + r / NJ, row = (long)first * NJ + r;
            float d = 0.f;
            if (located(a, b)) {
                float p[3], g[3];
                add_3(a.pred_cam + row * 3, a.tri + b * NJ * 3, p);
                add_3(a.gt_cam + row * 3, a.gt_root + b * 3, g);
                d = distance_3(p, g);
            }
            dist[r] = d;
        }
        __syncthreads();
        if (t < NJ)
            for (int s = 0; s < n; ++s)
                if (found[s]) col += (double)dist[s * NJ + t];
        if (t == NJ)
            for (int s = 0; s < n; ++s)
                if (found[s]) {
                    n_found += 1.0;
                    root_sum += (double)root_dist[s];
                }
        __syncthreads();
    }
    double *s = a.state;
    if (t < NJ) {
        s[kW + t] += col;
        column[t] = col;
    }
    __syncthreads();
    if (t == NJ) {
        double all = 0.0;
        for (int j = 0; j < NJ; ++j) all += column[j];
        s[0] += (double)a.B;
        s[1] += 1.0;
        s[2] = (double)a.V;
        s[3] += n_found;
        s[4] += all;
        s[5] += root_sum;
    }
}

// ---- workgroup 1: plain triangulation against the labels per joint, and the status counts
__device__ __forceinline__ void triangulated(const AbsoluteParams &a) {
    __shared__ float dist[kLanes * NJ];
    __shared__ uint8_t state_of[kLanes * NJ];   // the status clamped to 0 .. 3, plus 4 when the joint counts in T
    const int t = threadIdx.x;
    double sum = 0.0;
    long counted = 0, by_status[4] = {0, 0, 0, 0};
    for (int first = 0; first < a.B; first += kLanes) {
        const int n = min(kLanes, a.B - first);
        for (int r = t; r < n * NJ; r += kLanes) {
            const long b = first + r / NJ, row = (long)first * NJ + r;
            const int32_t st = a.status[row];
            const bool ok = st == 0 && finite_3(a.tri + row * 3);
            float d = 0.f;
            if (ok) {
                float g[3];
                add_3(a.gt_cam + row * 3, a.gt_root + b * 3, g);
                d = distance_3(a.tri + row * 3, g);
            }
            dist[r] = d;
            state_of[r] = (uint8_t)((st < 0 || st > 3 ? 3 : st) + (ok ? 4 : 0));
        }
        __syncthreads();
        if (t < NJ)
            for (int s = 0; s < n; ++s) {
                const int code = state_of[s * NJ + t];
                ++by_status[code & 3];
                if (code & 4) {
                    sum += (double)dist[s * NJ + t];
                    ++counted;
                }
            }
        __syncthreads();
    }
    if (t < NJ) {
        double *s = a.state;
        s[kT + t] += sum;
        s[kTN + t] += (double)counted;
        for (int k = 0; k < 4; ++k) s[kS + t * 4 + k] += (double)by_status[k];
    }
}

// ---- the reprojection error per camera over the joints with status 0: per camera a fixed lane-strided partial sum and a fixed tree
__device__ __forceinline__ void reprojection(const AbsoluteParams &a) {
    __shared__ double red[kLanes];
    const int t = threadIdx.x;
    const long rows = (long)a.B * NJ;
    for (int v = 0; v < a.V; ++v) {
        double sum = 0.0, count = 0.0;
        for (long r = t; r < rows; r += kLanes) {
            if (a.status[r] != 0) continue;
            const float e = a.reproj[((r / NJ) * a.V + v) * NJ + r % NJ];
            if (isfinite(e)) {
                sum += (double)e;
                count += 1.0;
            }
        }
        sum = block_sum<kLanes>(sum, red);
        count = block_sum<kLanes>(count, red);
        if (t == 0) {
            a.state[kFixed + v] += sum;
            a.state[kFixed + a.V + v] += count;
        }
    }
}

// ---- the inlier histogram over the joints with status 0: integer counts in LDS
__device__ __forceinline__ void inlier_histogram(const AbsoluteParams &a) {
    __shared__ unsigned long long hist[kMaxViews + 1];
    const int t = threadIdx.x;
    if (t <= kMaxViews) hist[t] = 0;
    __syncthreads();
    const long rows = (long)a.B * NJ;
    for (long r = t; r < rows; r += kLanes) {
        if (a.status[r] != 0) continue;
        const int32_t k = a.inliers[r];
        atomicAdd(&hist[k < 0 ? 0 : (k > a.V ? a.V : k)], 1ull);   // an integer count in LDS
    }
    __syncthreads();
    if (t <= a.V) a.state[kFixed + 2 * a.V + t] += (double)hist[t];
}

__global__ __launch_bounds__(kLanes) void eval_absolute_kernel(AbsoluteParams a) {
    // a state begun with another V: nothing is written (the entry has refused the call already unless its caller vouched for V).
    // Workgroup 0 writes [2] = V at its end; a workgroup that reads it then reads the value it compares with
    const double pinned = a.state[2];
    if (pinned != 0.0 && pinned != (double)a.V) return;
    const int role = blockIdx.x;
    if (role == 0)
        world(a);
    else if (role == 1)
        triangulated(a);
    else if (role == 2 && a.reproj)
        reprojection(a);
    else
        inlier_histogram(a);
}

using hmv::bad_arg;
using hmv::hip_fail;

}  // namespace

extern "C" size_t hmv_eval_absolute_doubles(int32_t V) { return V >= 1 && V <= kMaxViews ? (size_t)kFixed + 1 + 3 * (size_t)V : 0; }

extern "C" int hmv_eval_absolute_add(int32_t device, const hmv_eval_absolute_args *a, void *stream) {
    const char *who = "hmv_eval_absolute_add";
    if (!a) return bad_arg(who, "args is NULL");
    if (a->struct_size != (int32_t)sizeof(hmv_eval_absolute_args)) return bad_arg(who, "struct_size does not match this library's hmv_eval_absolute_args");
    if (a->B < 1) return bad_arg(who, "B must be >= 1");
    if (a->V < 1 || a->V > kMaxViews) return bad_arg(who, "V must be in 1 .. 16");
    if ((int64_t)a->B * a->V > (1 << 24)) return bad_arg(who, "B * V must not exceed 2^24 frames");
    if (!a->pred_joints_cam) return bad_arg(who, "pred_joints_cam is NULL");
    if (!a->joints_tri) return bad_arg(who, "joints_tri is NULL");
    if (!a->tri_status) return bad_arg(who, "tri_status is NULL");
    if (!a->gt_joints_cam) return bad_arg(who, "gt_joints_cam is NULL");
    if (!a->gt_root) return bad_arg(who, "gt_root is NULL");
    if (!a->state || ((uintptr_t)a->state & 7)) return bad_arg(who, "state is NULL or not 8-byte aligned");
    if (a->state_doubles < hmv_eval_absolute_doubles(a->V)) return bad_arg(who, "state_doubles is smaller than hmv_eval_absolute_doubles gives for V");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    // [2] pins the epoch's V: the slices behind the fixed part lie where V puts them.  Eight bytes read behind the stream's earlier
    // work, unless the caller has compared V on the host; the kernel compares in either case
    if (!a->v_checked) {
        double pinned = 0.0;
        if (hipMemcpyAsync(&pinned, a->state + 2, sizeof(double), hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
            hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
            return hip_fail(who, hipGetLastError());
        if (pinned != 0.0 && pinned != (double)a->V) return bad_arg(who, "V differs from the V this state was begun with (state[2])");
    }
    AbsoluteParams k;
    k.pred_cam = a->pred_joints_cam; k.tri = a->joints_tri; k.gt_cam = a->gt_joints_cam; k.gt_root = a->gt_root;
    k.reproj = a->reproj_err; k.status = a->tri_status; k.inliers = a->inliers; k.state = a->state;
    k.B = a->B; k.V = a->V;
    const int groups = 2 + (a->reproj_err ? 1 : 0) + (a->inliers ? 1 : 0);
    hipLaunchKernelGGL(eval_absolute_kernel, dim3(groups), dim3(kLanes), 0, (hipStream_t)stream, k);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}
