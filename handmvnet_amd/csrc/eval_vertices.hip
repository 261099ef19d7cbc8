// The mesh block of an evaluation epoch on the device: per step hmv_eval_vertices_add adds what HandMvNet._calculate_mpjpe
// (handmvnet.py:389-408) computes from the predicted and the labelled MANO vertices -- MPVPE, PA-MPVPE, the PCK curve of the vertex
// distances -- into a caller-owned fp64 state, next to the error of every vertex and one record row per sample (layouts:
// include/handmv.h, "vertex evaluation").
//
// The joint kernels (metrics.hip, eval_epoch.hip) align one pose per LANE, which suits 21 points.  A mesh has 778: here one WORKGROUP
// takes one sample and all of its lanes walk that sample's vertices.  Two launches:
//   mesh_kernel     grid of B workgroups.  Both meshes are divided by unit_div and staged in LDS once (24 n_verts bytes: a 12-byte
//                   vertex stride is 3 dwords, odd, so the 32 lanes of a bank group land on 32 banks), then read three times: distances,
//                   bins and the means; the centred moments; the aligned distances.  Lane 0 solves the 3x3 problem in between.  Per
//                   sample it leaves dist[v], pa_dist[v] and the partials {sum, pa_sum, skipped, hist[S + 1]} in the scratch.
//   fold_kernel     1 + ceil(n_verts / 256) workgroups, each the only writer of its slice of the state.  Workgroup 0 adds the partials
//                   onto the scalars and the histogram sample by sample in row order, the others add dist and pa_dist onto PV and PVA,
//                   one lane per vertex, sample by sample in row order.
// Every add onto the state is one sample's value, in feed order: the state after a split has the same bits however the split was cut
// into batches.  A sample's partials come from its own workgroup alone -- fixed-order wave and workgroup reductions, no floating-point
// atomics -- so they depend neither on B nor on its row.  fp32 where the reference compares (the division, the distance, its bin), fp64
// for sums and the alignment, as in pose_rows.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/handmv.h"
#include "kernels.h"
#include "pose_rows.h"

namespace {

constexpr int kLanes = 256;              // lanes of a workgroup, four waves
constexpr int kWaves = kLanes / 64;
constexpr int kMaxVerts = 4096, kMaxBatch = 4096;
constexpr int kScalars = 8;              // state[0 .. 8)
constexpr int kPartHead = 3;             // a sample's partials: sum, pa_sum, skipped, then hist[S + 1]
constexpr int kMaxSums = 10;             // values reduced together: var1 and the nine entries of K
// dynamic LDS of mesh_kernel: red[kMaxSums][kWaves] and xf[16] doubles, thr[256] floats, hist[257 (+ 3)] ints, then the two meshes
constexpr size_t kLdsHead = (kMaxSums * kWaves + 16) * sizeof(double) + kMaxSteps * sizeof(float) + (kMaxSteps + 4) * sizeof(int);
static_assert(kLdsHead % 16 == 0, "the meshes start on a 16-byte boundary");
static_assert(kMaxSteps == hmv::kMaxEvalSteps, "the LDS tables hold what the argument check lets through");
constexpr size_t lds_bytes(int n_verts) { return kLdsHead + (size_t)n_verts * 6 * sizeof(float); }

struct VertexParams {
    const float *pred, *gt;
    const int32_t *status;
    double *state, *part, *pa_dist;   // part: [B][kPartHead + S + 1]; pa_dist: [B][n]
    float *dist, *records;            // dist: [B][n]; records: [cap][2] or null
    long record_base;
    int B, n, steps;
    float tmin, tmax, unit_div;
};

// Sums of K values over the workgroup, every lane gets them: a shuffle tree inside each wave, then the four wave sums in wave order.
// red: K * kWaves doubles of LDS.  The order is a function of the lane alone.
template <int K>
__device__ __forceinline__ void group_sums(double (&v)[K], double *red) {
    for (int k = 0; k < K; ++k)
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
    const int t = threadIdx.x;
    __syncthreads();   // the previous call's readers are through
    if ((t & 63) == 0)
        for (int k = 0; k < K; ++k) red[k * kWaves + (t >> 6)] = v[k];
    __syncthreads();
    for (int k = 0; k < K; ++k) v[k] = ((red[k * kWaves] + red[k * kWaves + 1]) + red[k * kWaves + 2]) + red[k * kWaves + 3];
}

__global__ __launch_bounds__(kLanes) void mesh_kernel(VertexParams a) {
    extern __shared__ __attribute__((aligned(16))) char vsm[];
    double *red = reinterpret_cast<double *>(vsm);
    double *xf = red + kMaxSums * kWaves;                      // R [9], scale, tr [3]
    float *thr = reinterpret_cast<float *>(xf + 16);
    int *hist = reinterpret_cast<int *>(thr + kMaxSteps);
    float *P = reinterpret_cast<float *>(vsm + kLdsHead), *G = P + (size_t)a.n * 3;
    const int t = threadIdx.x, n = a.n, bins = a.steps + 1;
    const long b = blockIdx.x;
    double *part = a.part + b * (kPartHead + bins);
    float *rec = a.records ? a.records + (a.record_base + b) * 2 : nullptr;

    if (a.status && a.status[b] != 0) {   // uniform over the workgroup: a skipped sample's vertices are not read
        if (t == 0) {
            part[0] = 0.0;
            part[1] = 0.0;
            part[2] = 1.0;
            if (rec) rec[0] = rec[1] = NAN;
        }
        return;
    }

    fill_thresholds(thr, a.tmin, a.tmax, a.steps);
    for (int i = t; i < bins; i += kLanes) hist[i] = 0;
    const float *pred = a.pred + b * n * 3, *gt = a.gt + b * n * 3;
    for (int i = t; i < n * 3; i += kLanes) {   // the reference's `vertices / 1000.`, once for the three passes
        P[i] = pred[i] / a.unit_div;
        G[i] = gt[i] / a.unit_div;
    }
    __syncthreads();

    // ---- pass 1: the fp32 distance (the joint path's bits), its bin, and the six sums of the means
    double s1[7] = {0, 0, 0, 0, 0, 0, 0};
    for (int v = t; v < n; v += kLanes) {
        const float d = distance_3(P + v * 3, G + v * 3);
        a.dist[b * n + v] = d;
        s1[0] += (double)d;
        atomicAdd(&hist[threshold_bin(d, thr, a.steps)], 1);   // an integer count in LDS
        for (int c = 0; c < 3; ++c) {
            s1[1 + c] += (double)P[v * 3 + c];
            s1[4 + c] += (double)G[v * 3 + c];
        }
    }
    group_sums<7>(s1, red);
    PoseMoments m;
    for (int c = 0; c < 3; ++c) {
        m.mu1[c] = s1[1 + c] / n;
        m.mu2[c] = s1[4 + c] / n;
    }

    // ---- pass 2: the variance of the prediction and the cross-covariance, on centred values as pose_moments takes them
    double s2[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int v = t; v < n; v += kLanes) {
        double x1[3], x2[3];
        for (int c = 0; c < 3; ++c) {
            x1[c] = P[v * 3 + c] - m.mu1[c];
            x2[c] = G[v * 3 + c] - m.mu2[c];
            s2[0] += x1[c] * x1[c];
        }
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) s2[1 + i * 3 + j] += x1[i] * x2[j];
    }
    group_sums<10>(s2, red);

    // ---- one lane: the 3x3 problem, then R, scale and t for everyone
    if (t == 0) {
        m.var1 = s2[0];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) m.K[i][j] = s2[1 + i * 3 + j];
        double U[3][3], S[3], V[3][3], R[3][3], scale, tr[3];
        svd3(m.K, U, S, V);
        pose_similarity(m, U, V, R, scale, tr);
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) xf[i * 3 + j] = R[i][j];
            xf[10 + i] = tr[i];
        }
        xf[9] = scale;
    }
    __syncthreads();
    double R[3][3], tr[3];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) R[i][j] = xf[i * 3 + j];
        tr[i] = xf[10 + i];
    }
    const double scale = xf[9];

    // ---- pass 3: what remains after the alignment
    double s3[1] = {0};
    for (int v = t; v < n; v += kLanes) {
        double y[3];
        const double d = pose_aligned_distance(P + v * 3, G + v * 3, R, scale, tr, y);
        a.pa_dist[b * n + v] = d;
        s3[0] += d;
    }
    group_sums<1>(s3, red);   // its barriers also complete hist

    for (int i = t; i < bins; i += kLanes) part[kPartHead + i] = (double)hist[i];
    if (t == 0) {
        part[0] = s1[0];
        part[1] = s3[0];
        part[2] = 0.0;
        if (rec) {
            rec[0] = (float)(s1[0] / n);
            rec[1] = (float)(s3[0] / n);
        }
    }
}

__global__ __launch_bounds__(kLanes) void fold_kernel(VertexParams a) {
    const int t = threadIdx.x, n = a.n, bins = a.steps + 1, stride = kPartHead + bins;
    double *s = a.state;
    if (blockIdx.x == 0) {
        for (int i = t; i < bins; i += kLanes) {   // each bin by one lane, down the samples
            double h = s[kScalars + i];
            for (int b = 0; b < a.B; ++b)
                if (a.part[(long)b * stride + 2] == 0.0) h += a.part[(long)b * stride + kPartHead + i];
            s[kScalars + i] = h;
        }
        if (t == 0) {
            double sum = s[6], pa = s[7];
            int added = 0;
            for (int b = 0; b < a.B; ++b) {
                const double *p = a.part + (long)b * stride;
                if (p[2] != 0.0) continue;
                sum += p[0];
                pa += p[1];
                ++added;
            }
            if (s[1] == 0.0) {
                s[2] = (double)n;
                s[3] = (double)a.steps;
            }
            s[0] += (double)added;
            s[1] += 1.0;
            s[4] += (double)(a.B - added);
            s[5] += (double)added * (double)n;
            s[6] = sum;
            s[7] = pa;
        }
        return;
    }
    const int v = (blockIdx.x - 1) * kLanes + t;
    if (v >= n) return;
    double *PV = s + kScalars + bins, *PVA = PV + n;
    double pv = PV[v], pva = PVA[v];
    for (int b = 0; b < a.B; ++b) {
        if (a.part[(long)b * stride + 2] != 0.0) continue;   // the same address for every lane
        pv += (double)a.dist[(long)b * n + v];
        pva += a.pa_dist[(long)b * n + v];
    }
    PV[v] = pv;
    PVA[v] = pva;
}

using hmv::bad_arg;
using hmv::hip_fail;

bool shape_ok(int B, int n, int steps) { return B >= 1 && B <= kMaxBatch && n >= 1 && n <= kMaxVerts && steps >= 1 && steps <= kMaxSteps; }

}  // namespace

extern "C" size_t hmv_eval_vertices_doubles(int32_t n_verts, int32_t steps) {
    return shape_ok(1, n_verts, steps) ? (size_t)kScalars + (steps + 1) + 2 * (size_t)n_verts : 0;
}

extern "C" size_t hmv_eval_vertices_scratch_bytes(int32_t B, int32_t n_verts, int32_t steps) {
    if (!shape_ok(B, n_verts, steps)) return 0;
    return (size_t)B * ((kPartHead + steps + 1) * sizeof(double) + (size_t)n_verts * (sizeof(double) + sizeof(float)));
}

extern "C" int hmv_eval_vertices_add(int32_t device, const hmv_eval_vertices_args *a, void *stream) {
    const char *who = "hmv_eval_vertices_add";
    if (!a) return bad_arg(who, "args is NULL");
    if (a->struct_size != (int32_t)sizeof(hmv_eval_vertices_args)) return bad_arg(who, "struct_size does not match this library's hmv_eval_vertices_args");
    if (a->B < 1 || a->B > kMaxBatch) return bad_arg(who, "B must be in 1 .. 4096");
    if (a->n_verts < 1 || a->n_verts > kMaxVerts) return bad_arg(who, "n_verts must be in 1 .. 4096");
    if (a->steps < 1 || a->steps > kMaxSteps) return bad_arg(who, "steps must be in 1 .. 256");
    if (!(a->thr_max >= a->thr_min)) return bad_arg(who, "thr_max must not be below thr_min");
    if (!(a->unit_div > 0.f) || !isfinite(a->unit_div)) return bad_arg(who, "unit_div must be finite and > 0");
    if (!a->pred_vertices) return bad_arg(who, "pred_vertices is NULL");
    if (!a->gt_vertices) return bad_arg(who, "gt_vertices is NULL");
    if ((uintptr_t)a->status & 3) return bad_arg(who, "status is not 4-byte aligned");
    if (!a->state || ((uintptr_t)a->state & 7)) return bad_arg(who, "state is NULL or not 8-byte aligned");
    if (a->state_doubles < hmv_eval_vertices_doubles(a->n_verts, a->steps))
        return bad_arg(who, "state_doubles is smaller than hmv_eval_vertices_doubles gives for n_verts and steps");
    if (!a->scratch || ((uintptr_t)a->scratch & 7)) return bad_arg(who, "scratch is NULL or not 8-byte aligned");
    if (a->scratch_bytes < hmv_eval_vertices_scratch_bytes(a->B, a->n_verts, a->steps))
        return bad_arg(who, "scratch_bytes is smaller than hmv_eval_vertices_scratch_bytes gives for B, n_verts and steps");
    if (a->records) {
        if ((uintptr_t)a->records & 3) return bad_arg(who, "records is not 4-byte aligned");
        if (a->record_capacity < 1) return bad_arg(who, "record_capacity must be >= 1 with records");
        if (a->record_base < 0) return bad_arg(who, "record_base must be >= 0");
        if (a->record_base > a->record_capacity - a->B) return bad_arg(who, "record_base + B exceeds record_capacity");
    }
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    static hmv::DeviceOnce once;   // a mesh beyond 2600 vertices takes more LDS than a kernel gets unasked
    hipError_t e = once.run([&](int) { return hmv::set_max_lds(lds_bytes(kMaxVerts), mesh_kernel); });
    if (e != hipSuccess) return hip_fail(who, e);
    VertexParams k;
    k.pred = a->pred_vertices; k.gt = a->gt_vertices; k.status = a->status; k.state = a->state;
    k.B = a->B; k.n = a->n_verts; k.steps = a->steps;
    k.tmin = a->thr_min; k.tmax = a->thr_max; k.unit_div = a->unit_div;
    k.records = a->records; k.record_base = a->records ? (long)a->record_base : 0;
    k.part = static_cast<double *>(a->scratch);                         // doubles first: every slice keeps its alignment
    k.pa_dist = k.part + (size_t)a->B * (kPartHead + a->steps + 1);
    k.dist = reinterpret_cast<float *>(k.pa_dist + (size_t)a->B * a->n_verts);
    hipLaunchKernelGGL(mesh_kernel, dim3(a->B), dim3(kLanes), lds_bytes(a->n_verts), (hipStream_t)stream, k);
    if ((e = hipGetLastError()) != hipSuccess) return hip_fail(who, e);
    hipLaunchKernelGGL(fold_kernel, dim3(1 + (a->n_verts + kLanes - 1) / kLanes), dim3(kLanes), 0, (hipStream_t)stream, k);
    e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}
