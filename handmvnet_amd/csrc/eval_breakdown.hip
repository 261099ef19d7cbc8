// The breakdown of an evaluation epoch on the device: per step ONE launch adds, next to the pooled sums of eval_epoch.hip, the same
// errors kept apart by joint, by camera and -- optionally -- by sample, into a second caller-owned fp64 state and a table of fp32
// record rows (layouts: include/handmv.h, "evaluation breakdown").
//
// Built from the device functions of pose_rows.h like the epoch kernels: fp32 for the distance-versus-threshold comparison, fp64 for
// sums and the 3x3 Procrustes problem, no floating-point atomics, every sum in a fixed order.  A few workgroups, each the only
// writer of its slice of the state, so nothing needs an atomic on memory:
//   workgroup 0          J3, H and the header; record column 0 (the sample's MPJPE)
//   workgroup 1          JPA, one lane per pose; record column 1
//   workgroup 2 + v      CN[v], C2[v], CV[v] of camera v; record column 4 + v
//   workgroup 2 + V      only with records: columns 2 and 3 (the sample's own 2D MPJPE over its present views, and their number)
// Samples are taken in chunks of kLanes.  A chunk's per-row values are staged in LDS; lane j < 21 then adds column j down the chunk
// in sample order, lane s adds row s along the joints for the record.  Each workgroup read-modify-writes its slice at the end in
// plain C++; stream order orders successive steps.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/handmv.h"
#include "kernels.h"
#include "pose_rows.h"

namespace {

constexpr int kLanes = 256;    // lanes of a workgroup and samples of a staged chunk.  256 and not the epoch kernels' 1024: the alignment lane
                               // then has 512 registers to itself (eval_epoch.hip explains what 1024 lanes leave it)
constexpr int kHeader = 4;     // state[0 .. 4): samples, steps added, V, S
constexpr int kRecordHead = 4; // record row: mpjpe, pa_mpjpe, mpjpe2d, views, then one value per camera

struct BreakdownParams {
    const float *pred_cam, *gt_cam, *pred_2d, *gt_2d;
    const uint8_t *mask, *present;
    double *state;
    float *records;
    long record_base;
    int B, V, steps;
    float tmin, tmax;
};

__device__ __forceinline__ float *record_row(const BreakdownParams &a, long sample) {
    return a.records + (a.record_base + sample) * (long)(kRecordHead + a.V);
}

// the masked 2D distance of row r = (sample * V + view) * 21 + joint: a masked joint is zeroed on both sides (eval_epoch.hip)
__device__ __forceinline__ float distance_2d(const BreakdownParams &a, long r, bool *visible) {
    const float keep = (a.mask && a.mask[r]) ? 0.f : 1.f;
    const float p[2] = {a.pred_2d[r * 2] * keep, a.pred_2d[r * 2 + 1] * keep};
    const float g[2] = {a.gt_2d[r * 2] * keep, a.gt_2d[r * 2 + 1] * keep};
    *visible = keep != 0.f;
    return distance_2(p, g);
}

// ---- workgroup 0: the 3D distance per joint, its PCK bins per joint, the header
__device__ __forceinline__ void joints_3d(const BreakdownParams &a) {
    __shared__ float thr[kMaxSteps];
    __shared__ int hist[NJ * (kMaxSteps + 1)];
    __shared__ float dist[kLanes * NJ];
    const int t = threadIdx.x, bins = a.steps + 1;
    fill_thresholds(thr, a.tmin, a.tmax, a.steps);
    for (int i = t; i < NJ * bins; i += kLanes) hist[i] = 0;
    __syncthreads();
    double col = 0.0;   // lane j < 21: joint j down the samples
    for (int first = 0; first < a.B; first += kLanes) {
        const int n = min(kLanes, a.B - first);
        for (int r = t; r < n * NJ; r += kLanes) {
            const long row = (long)first * NJ + r;
            const float d = distance_3(a.pred_cam + row * 3, a.gt_cam + row * 3);
            dist[r] = d;
            atomicAdd(&hist[(r % NJ) * bins + threshold_bin(d, thr, a.steps)], 1);   // an integer count in LDS
        }
        __syncthreads();
        if (t < NJ)
            for (int s = 0; s < n; ++s) col += (double)dist[s * NJ + t];
        if (a.records && t < n) {
            double m = 0.0;
            for (int j = 0; j < NJ; ++j) m += (double)dist[t * NJ + j];
            record_row(a, first + t)[0] = (float)(m / NJ);
        }
        __syncthreads();
    }
    double *s = a.state;
    if (t < NJ) s[kHeader + t] += col;
    double *H = s + kHeader + 2 * NJ;
    for (int i = t; i < NJ * bins; i += kLanes) H[i] += (double)hist[i];
    if (t == 0) {
        if (s[1] == 0.0) {
            s[2] = (double)a.V;
            s[3] = (double)a.steps;
        }
        s[0] += (double)a.B;
        s[1] += 1.0;
    }
}

// ---- workgroup 1: the distance per joint that remains after each pose's similarity alignment, one lane per pose
__device__ __forceinline__ void joints_aligned(const BreakdownParams &a) {
    __shared__ double dist[kLanes * NJ];
    const int t = threadIdx.x;
    double col = 0.0;
    for (int first = 0; first < a.B; first += kLanes) {   // a uniform counter, as in eval_epoch.hip
        const int n = min(kLanes, a.B - first);
        if (t < n) {
            const float *p = a.pred_cam + (long)(first + t) * NJ * 3, *g = a.gt_cam + (long)(first + t) * NJ * 3;
            PoseMoments m;
            pose_moments(p, g, NJ, m);
            double U[3][3], S[3], V[3][3];
            svd3(m.K, U, S, V);
            double *out = dist + t * NJ;
            pose_aligned_points(p, g, NJ, m, U, V, [&](int j, const double *, double d) { out[j] = d; });
        }
        __syncthreads();
        if (t < NJ)
            for (int s = 0; s < n; ++s) col += dist[s * NJ + t];
        if (a.records && t < n) {
            double m = 0.0;
            for (int j = 0; j < NJ; ++j) m += dist[t * NJ + j];
            record_row(a, first + t)[1] = (float)(m / NJ);
        }
        __syncthreads();
    }
    if (t < NJ) a.state[kHeader + NJ + t] += col;
}

// ---- workgroup 2 + v: camera v.  An absent slot is not read: it adds 0 to every sum and NaN to its record
__device__ __forceinline__ void camera_2d(const BreakdownParams &a, int v) {
    __shared__ float dist[kLanes * NJ];
    __shared__ uint8_t seen[kLanes * NJ];   // 1: the slot is present and the joint not masked
    __shared__ uint8_t here[kLanes];        // 1: the slot is present
    const int t = threadIdx.x;
    double c2 = 0.0, cv = 0.0, cn = 0.0;    // lane j < 21: C2[v][j], CV[v][j]; lane 21: CN[v]
    for (int first = 0; first < a.B; first += kLanes) {
        const int n = min(kLanes, a.B - first);
        if (t < n) here[t] = !a.present || a.present[(long)(first + t) * a.V + v];
        for (int r = t; r < n * NJ; r += kLanes) {
            const long slot = (long)(first + r / NJ) * a.V + v;
            float d = 0.f;
            bool visible = false;
            if (!a.present || a.present[slot]) d = distance_2d(a, slot * NJ + r % NJ, &visible);
            dist[r] = d;
            seen[r] = visible;
        }
        __syncthreads();
        if (t < NJ)
            for (int s = 0; s < n; ++s) {
                c2 += (double)dist[s * NJ + t];
                cv += (double)seen[s * NJ + t];
            }
        if (t == NJ)
            for (int s = 0; s < n; ++s) cn += (double)here[s];
        if (a.records && t < n) {
            double m = 0.0;
            for (int j = 0; j < NJ; ++j) m += (double)dist[t * NJ + j];
            record_row(a, first + t)[kRecordHead + v] = here[t] ? (float)(m / NJ) : NAN;
        }
        __syncthreads();
    }
    double *CN = a.state + kHeader + 2 * NJ + NJ * (a.steps + 1), *C2 = CN + a.V, *CV = C2 + (long)a.V * NJ;
    if (t < NJ) {
        C2[v * NJ + t] += c2;
        CV[v * NJ + t] += cv;
    }
    if (t == NJ) CN[v] += cn;
}

// ---- workgroup 2 + V (records only): one lane per sample walks its present views.  No view at all: 0 / 0 = NaN
__device__ __forceinline__ void sample_2d(const BreakdownParams &a) {
    for (int b = threadIdx.x; b < a.B; b += kLanes) {
        int views = 0;
        double sum = 0.0;
        for (int v = 0; v < a.V; ++v) {
            const long slot = (long)b * a.V + v;
            if (a.present && !a.present[slot]) continue;
            ++views;
            for (int j = 0; j < NJ; ++j) {
                bool visible;
                sum += (double)distance_2d(a, slot * NJ + j, &visible);
            }
        }
        float *rec = record_row(a, b);
        rec[2] = (float)(sum / (double)(views * NJ));
        rec[3] = (float)views;
    }
}

__global__ __launch_bounds__(kLanes) void eval_breakdown_kernel(BreakdownParams a) {
    const int role = blockIdx.x;
    if (role == 0)
        joints_3d(a);
    else if (role == 1)
        joints_aligned(a);
    else if (role < 2 + a.V)
        camera_2d(a, role - 2);
    else
        sample_2d(a);
}

using hmv::bad_arg;
using hmv::hip_fail;

}  // namespace

extern "C" size_t hmv_eval_breakdown_doubles(int32_t V, int32_t steps) {
    if (V < 1 || steps < 1 || steps > kMaxSteps) return 0;
    return (size_t)kHeader + 2 * NJ + (size_t)NJ * (steps + 1) + (size_t)V * (1 + 2 * NJ);
}

extern "C" size_t hmv_eval_record_floats(int32_t V) { return V >= 1 ? (size_t)kRecordHead + V : 0; }

extern "C" int hmv_eval_breakdown_add(int32_t device, const hmv_eval_breakdown_args *a, void *stream) {
    const char *who = "hmv_eval_breakdown_add";
    if (const int rc = hmv::check_eval_args(who, a, "hmv_eval_breakdown_args", a ? hmv_eval_breakdown_doubles(a->V, a->steps) : 0,
                                            "state_doubles is smaller than hmv_eval_breakdown_doubles gives for V and steps"))
        return rc;
    if (a->records) {
        if ((uintptr_t)a->records & 3) return bad_arg(who, "records is not 4-byte aligned");
        if (a->record_capacity < 1) return bad_arg(who, "record_capacity must be >= 1 with records");
        if (a->record_base < 0) return bad_arg(who, "record_base must be >= 0");
        if (a->record_base > a->record_capacity - a->B) return bad_arg(who, "record_base + B exceeds record_capacity");
    }
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    BreakdownParams k;
    k.pred_cam = a->pred_joints_cam; k.gt_cam = a->gt_joints_cam; k.pred_2d = a->pred_joints_2d; k.gt_2d = a->gt_joints_2d;
    k.mask = a->joints_mask; k.present = a->view_present; k.state = a->state;
    k.records = a->records; k.record_base = a->records ? (long)a->record_base : 0;
    k.B = a->B; k.V = a->V; k.steps = a->steps;
    k.tmin = a->thr_min; k.tmax = a->thr_max;
    const int groups = 2 + a->V + (a->records ? 1 : 0);
    hipLaunchKernelGGL(eval_breakdown_kernel, dim3(groups), dim3(kLanes), 0, (hipStream_t)stream, k);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}
