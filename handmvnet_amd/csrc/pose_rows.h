// Device code shared by the evaluation kernels (metrics.hip: one step's metrics; eval_epoch.hip: an epoch's running sums;
// eval_breakdown.hip: the same by joint, camera and sample; eval_vertices.hip: the mesh block, one workgroup per mesh; losses.hip: the
// step's losses; hand_ik.hip uses svd3, pose_consensus.hip solve4_xyz), as functions, so that they cannot drift apart: the workgroup reduction, the 3x3 SVD, the 4x4 cofactor solve of the
// camera-to-camera transforms, the present-view count of a ragged sample, and the per-row
// arithmetic of models/metrics.py -- thresholds as torch.linspace builds them, the fp32 joint distance, its PCK bin, the similarity
// alignment of one pose.  The arithmetic that decides a comparison (joint distance vs threshold) is fp32 like the reference's and
// written out under contract(off): its roundings are the source's, not the optimiser's.  Sums and the 3x3 Procrustes problem run
// in fp64.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace {

constexpr int NJ = 21;
constexpr int kMaxSteps = 256;
constexpr int kCountSlots = 1024;   // samples whose present-view count is kept in LDS; a sample beyond them has its mask row counted when asked

// Fixed-order tree reduction over a workgroup of N lanes (red: N doubles of LDS); every lane gets the total.
template <int N>
__device__ double block_sum(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}

// One-sided Jacobi (Hestenes) SVD of a 3x3 matrix: a = u * diag(s) * v^T, s descending.
// A column of u that belongs to a zero singular value is completed with the cross product of the others.
[[maybe_unused]] __device__ void svd3(const double a[3][3], double u[3][3], double s[3], double v[3][3]) {
    double w[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            w[i][j] = a[i][j];
            v[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0, be = 0, ga = 0;
                for (int i = 0; i < 3; ++i) {
                    al += w[i][p] * w[i][p];
                    be += w[i][q] * w[i][q];
                    ga += w[i][p] * w[i][q];
                }
                if (fabs(ga) <= 1e-300 || fabs(ga) <= 1e-17 * sqrt(al * be)) continue;
                off = fmax(off, fabs(ga) / sqrt(al * be));
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
                for (int i = 0; i < 3; ++i) {
                    const double wp = w[i][p], wq = w[i][q];
                    w[i][p] = c * wp - sn * wq;
                    w[i][q] = sn * wp + c * wq;
                    const double vp = v[i][p], vq = v[i][q];
                    v[i][p] = c * vp - sn * vq;
                    v[i][q] = sn * vp + c * vq;
                }
            }
        if (off < 1e-15) break;
    }
    double n[3];
    for (int j = 0; j < 3; ++j) n[j] = sqrt(w[0][j] * w[0][j] + w[1][j] * w[1][j] + w[2][j] * w[2][j]);
    int ord[3] = {0, 1, 2};
    for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2 - i; ++j)
            if (n[ord[j]] < n[ord[j + 1]]) {
                const int tmp = ord[j];
                ord[j] = ord[j + 1];
                ord[j + 1] = tmp;
            }
    double vs[3][3];
    for (int j = 0; j < 3; ++j) {
        const int o = ord[j];
        s[j] = n[o];
        for (int i = 0; i < 3; ++i) {
            vs[i][j] = v[i][o];
            u[i][j] = n[o] > 0 ? w[i][o] / n[o] : 0.0;
        }
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v[i][j] = vs[i][j];
    const double tiny = 1e-14 * s[0];
    if (s[2] <= tiny) {
        if (s[1] <= tiny) {   // rank <= 1: any orthonormal completion
            int k = 0;
            if (s[0] > 0) {
                for (int i = 1; i < 3; ++i)
                    if (fabs(u[i][0]) < fabs(u[k][0])) k = i;
            } else {
                u[0][0] = 1; u[1][0] = 0; u[2][0] = 0;
                k = 1;
            }
            double e[3] = {0, 0, 0};
            e[k] = 1.0;
            const double d = e[0] * u[0][0] + e[1] * u[1][0] + e[2] * u[2][0];
            double nn = 0;
            for (int i = 0; i < 3; ++i) {
                u[i][1] = e[i] - d * u[i][0];
                nn += u[i][1] * u[i][1];
            }
            nn = sqrt(nn);
            for (int i = 0; i < 3; ++i) u[i][1] /= nn;
        }
        u[0][2] = u[1][0] * u[2][1] - u[2][0] * u[1][1];
        u[1][2] = u[2][0] * u[0][1] - u[0][0] * u[2][1];
        u[2][2] = u[0][0] * u[1][1] - u[1][0] * u[0][1];
    }
}

[[maybe_unused]] __device__ double det3(const double m[3][3]) {
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

// Rows 0..2 of inverse(a) * b for a general 4x4 `a` (row-major): cofactor expansion over 2x2 minors, no pivoting needed and no
// dynamic indexing.  det == 0 gives inf / NaN.  (hmv_project_joints and the losses' reprojection, losses.hip; the camera-to-camera
// rotation of pose_consensus.hip.)
[[maybe_unused]] __device__ void solve4_xyz(const double a[16], const double b[4], double y[3]) {
    const double s0 = a[0] * a[5] - a[4] * a[1], s1 = a[0] * a[6] - a[4] * a[2], s2 = a[0] * a[7] - a[4] * a[3];
    const double s3 = a[1] * a[6] - a[5] * a[2], s4 = a[1] * a[7] - a[5] * a[3], s5 = a[2] * a[7] - a[6] * a[3];
    const double c5 = a[10] * a[15] - a[14] * a[11], c4 = a[9] * a[15] - a[13] * a[11], c3 = a[9] * a[14] - a[13] * a[10];
    const double c2 = a[8] * a[15] - a[12] * a[11], c1 = a[8] * a[14] - a[12] * a[10], c0 = a[8] * a[13] - a[12] * a[9];
    const double det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
    const double i00 = a[5] * c5 - a[6] * c4 + a[7] * c3, i01 = -a[1] * c5 + a[2] * c4 - a[3] * c3;
    const double i02 = a[13] * s5 - a[14] * s4 + a[15] * s3, i03 = -a[9] * s5 + a[10] * s4 - a[11] * s3;
    const double i10 = -a[4] * c5 + a[6] * c2 - a[7] * c1, i11 = a[0] * c5 - a[2] * c2 + a[3] * c1;
    const double i12 = -a[12] * s5 + a[14] * s2 - a[15] * s1, i13 = a[8] * s5 - a[10] * s2 + a[11] * s1;
    const double i20 = a[4] * c4 - a[5] * c2 + a[7] * c0, i21 = -a[0] * c4 + a[1] * c2 - a[3] * c0;
    const double i22 = a[12] * s4 - a[13] * s2 + a[15] * s0, i23 = -a[8] * s4 + a[9] * s2 - a[11] * s0;
    y[0] = (i00 * b[0] + i01 * b[1] + i02 * b[2] + i03 * b[3]) / det;
    y[1] = (i10 * b[0] + i11 * b[1] + i12 * b[2] + i13 * b[3]) / det;
    y[2] = (i20 * b[0] + i21 * b[1] + i22 * b[2] + i23 * b[3]) / det;
}

// get_2d_joints_from_3d_joints for one joint of one view (camera.py:4-60), then optionally the crop mapping
// (datasets/utils.py:124-143 with its default image_size of 256).  x3: the joint in camera `root` (metres), root3: added to it
// first when given.  e_root / e_view: [4][4] extrinsics, k: fx, fy, cx, cy, box: x1, y1, x2, y2 or null.  depth, when given, receives
// the depth term the division used: millimetres plus the reference's epsilon.  (hmv_project_joints and the losses' reprojection,
// losses.hip; the windows from the reprojected pose, track.hip.)
// This function is compiled with the compiler's default contraction (track.hip includes this header in front of its contract(off)
// pragma for that reason), so which products are fused is the optimiser's choice.  That hmv_op_reproject_crop_boxes' joints_reproj has
// hmv_project_joints' bits rests on it choosing alike in both kernels, whose inlining contexts differ (a null root3 and box and a
// depth there); nothing in the source guarantees it, tests/test_gpu_reproject_track.py asserts it.  If a compiler ever breaks it, pin
// the roundings here under contract(off), as distance_3 below does, and accept that hmv_project_joints' last bits move once.
[[maybe_unused]] __device__ void project_joint(const float *__restrict__ x3, const float *__restrict__ root3, const float *__restrict__ e_root,
                                               const float *__restrict__ e_view, const float *__restrict__ k, const float *__restrict__ box,
                                               double &u, double &v, double *depth = nullptr) {
    double X[3];
    for (int c = 0; c < 3; ++c) X[c] = (double)x3[c] + (root3 ? (double)root3[c] : 0.0);
    double xw[4], a[16], y[3];
    for (int r = 0; r < 4; ++r)
        xw[r] = (double)e_root[r * 4] * X[0] + (double)e_root[r * 4 + 1] * X[1] + (double)e_root[r * 4 + 2] * X[2] + (double)e_root[r * 4 + 3];
    for (int i = 0; i < 16; ++i) a[i] = (double)e_view[i];
    solve4_xyz(a, xw, y);
    const double z = y[2] * 1000.0 + 1e-6;
    u = y[0] * 1000.0 * (double)k[0] / z + (double)k[2];
    v = y[1] * 1000.0 * (double)k[1] / z + (double)k[3];
    if (box) {
        u = (u - (double)box[0]) * (256.0 / ((double)box[2] - (double)box[0]));
        v = (v - (double)box[1]) * (256.0 / ((double)box[3] - (double)box[1]));
    }
    if (depth) *depth = z;
}

// Rows 0..2 of inverse(e) for a row-major 4x4: solve4_xyz on the four unit vectors, so T[r][k] is cofactor / det exactly (the products
// with 1 and the sums with 0 round nothing).  A singular e gives inf / NaN.  (pose_consensus.hip, triangulate.hip.)
[[maybe_unused]] __device__ __forceinline__ void inverse_rows(const float *__restrict__ e, double T[3][4]) {
    double a[16];
    for (int i = 0; i < 16; ++i) a[i] = (double)e[i];
    for (int k = 0; k < 4; ++k) {
        const double unit[4] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0, k == 3 ? 1.0 : 0.0};
        double col[3];
        solve4_xyz(a, unit, col);
        for (int r = 0; r < 3; ++r) T[r][k] = col[r];
    }
}

// thr[0 .. steps) = torch.linspace(tmin, tmax, steps) in fp32: symmetric fill from both ends, one fma per value (metrics.py:105).
// Lanes 0 .. steps - 1 write one value each; the caller synchronises.
__device__ __forceinline__ void fill_thresholds(float* thr, float tmin, float tmax, int steps) {
    const int t = threadIdx.x;
    if (t < steps) {
        const float step = steps > 1 ? (tmax - tmin) / (float)(steps - 1) : 0.f;
        thr[t] = t < steps / 2 ? fmaf(step, (float)t, tmin) : fmaf(-step, (float)(steps - 1 - t), tmax);
        if (steps == 1) thr[t] = tmin;
    }
}

// |p - g| in fp32 (metrics.py:12, 77).  A distance is compared with a threshold, and a last-bit difference moves it into another PCK
// bin, so every multiply-add below is spelled out under contract(off): which squares are rounded on their own and which are fused is
// stated here and no longer picked by the optimiser from what surrounds a call.  The forms are the ones this library has always
// computed (what the kernels compiled to before they were pinned); they differ in the last bit, so they stay apart:
//   distance_3, distance_2   the epoch kernels and the breakdown, whose sums and bins must agree with each other
//   distance_n               pose_metrics_kernel, whose `dim` (1 .. 4) is a run-time value: a chain of fmas from 0, so at dim 3 its
//                            last square is fused where distance_3 rounds it
__device__ __forceinline__ float distance_3(const float* p, const float* g) {
#pragma clang fp contract(off)
    const float d0 = p[0] - g[0], d1 = p[1] - g[1], d2 = p[2] - g[2];
    return sqrtf(fmaf(d1, d1, d0 * d0) + d2 * d2);
}

__device__ __forceinline__ float distance_2(const float* p, const float* g) {
#pragma clang fp contract(off)
    const float d0 = p[0] - g[0], d1 = p[1] - g[1];
    return sqrtf(d0 * d0 + d1 * d1);
}

__device__ __forceinline__ float distance_n(const float* p, const float* g, int dim) {
#pragma clang fp contract(off)
    float acc = 0.f;
    for (int c = 0; c < dim; ++c) {
        const float d = p[c] - g[c];
        acc = fmaf(d, d, acc);
    }
    return sqrtf(acc);
}

// PCK histogram bin of a distance: the first threshold with dist <= thr (thresholds ascend), `steps` when there is none
__device__ __forceinline__ int threshold_bin(float dist, const float* thr, int steps) {
    int b = 0;
    while (b < steps && !(dist <= thr[b])) ++b;
    return b;
}

// Present views of one sample of a ragged view set: its row of the view mask [B][V] (non-zero = the view is there), counted.
__device__ __forceinline__ int count_views(const uint8_t* __restrict__ row, int V) {
    int n = 0;
    for (int v = 0; v < V; ++v) n += row[v] != 0;
    return n;
}

// cnt[b] = the present views of sample b, for the first kCountSlots samples, by a workgroup of N lanes; the caller synchronises.
template <int N>
__device__ __forceinline__ void fill_view_counts(int* cnt, const uint8_t* __restrict__ present, int B, int V) {
    for (int b = threadIdx.x; b < B && b < kCountSlots; b += N) cnt[b] = count_views(present + (long)b * V, V);
}

// V / v_b, what a present row of sample b adds its value times so that the sum over all slots, divided by the uniform divisor, is the
// mean over samples of each sample's own mean over its v_b present views.  Exactly 1.0 for a full sample.  A sample without a present
// view (a broken precondition) gives V / 0 = inf; nothing is indexed by a count.
__device__ __forceinline__ double view_weight(const uint8_t* __restrict__ present, const int* cnt, long b, int V) {
    return (double)V / (double)(b < kCountSlots ? cnt[b] : count_views(present + b * V, V));
}

// The similarity transform of one predicted pose p [n_pts][3] onto its target g (metrics.py:128-176), in two pieces around
// svd3(m.K, U, S, V): the moments, and the transformed points.
struct PoseMoments {
    double mu1[3], mu2[3];   // the means of p and g
    double var1;             // the variance of p
    double K[3][3];          // the cross-covariance
};

__device__ __forceinline__ void pose_moments(const float* p, const float* g, int n_pts, PoseMoments& m) {
    for (int c = 0; c < 3; ++c) m.mu1[c] = m.mu2[c] = 0.0;
    for (int j = 0; j < n_pts; ++j)
        for (int c = 0; c < 3; ++c) {
            m.mu1[c] += p[j * 3 + c];
            m.mu2[c] += g[j * 3 + c];
        }
    for (int c = 0; c < 3; ++c) {
        m.mu1[c] /= n_pts;
        m.mu2[c] /= n_pts;
    }
    m.var1 = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) m.K[a][b] = 0.0;
    for (int j = 0; j < n_pts; ++j) {
        double x1[3], x2[3];
        for (int c = 0; c < 3; ++c) {
            x1[c] = p[j * 3 + c] - m.mu1[c];
            x2[c] = g[j * 3 + c] - m.mu2[c];
            m.var1 += x1[c] * x1[c];
        }
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) m.K[a][b] += x1[a] * x2[b];
    }
}

// From the moments and the U, V of svd3(m.K, ...): the rotation R, the scale and the translation tr of y = scale * R x + tr.
// (pose_aligned_points below, one lane per pose; eval_vertices.hip, where one lane computes them for a workgroup's mesh.)
__device__ __forceinline__ void pose_similarity(const PoseMoments& m, const double U[3][3], const double V[3][3], double R[3][3],
                                                double& scale, double tr[3]) {
    // Z = diag(1, 1, sign(det(U V^T)));  R = V Z U^T
    double UVt[3][3];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) UVt[a][b] = U[a][0] * V[b][0] + U[a][1] * V[b][1] + U[a][2] * V[b][2];
    const double dd = det3(UVt);
    const double z = dd > 0 ? 1.0 : (dd < 0 ? -1.0 : 0.0);
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) R[a][b] = V[a][0] * U[b][0] + V[a][1] * U[b][1] + z * V[a][2] * U[b][2];
    double trace = 0.0;   // trace(R K)
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) trace += R[a][b] * m.K[b][a];
    scale = trace / m.var1;
    for (int a = 0; a < 3; ++a) tr[a] = m.mu2[a] - scale * (R[a][0] * m.mu1[0] + R[a][1] * m.mu1[1] + R[a][2] * m.mu1[2]);
}

// The distance that remains between the transformed point y = scale * R p + tr and g, and y itself: the per-point arithmetic of
// pose_aligned_points for a caller that spreads the points over lanes (eval_vertices.hip).  pose_aligned_points keeps its own loop:
// routed through this function, pose_metrics_kernel and eval_breakdown_kernel come out in another instruction schedule; as it is,
// the device code of the three files that use it is what it was before the split, instruction for instruction (tools/isa_diff.py).
__device__ __forceinline__ double pose_aligned_distance(const float* p, const float* g, const double R[3][3], double scale,
                                                        const double tr[3], double y[3]) {
    double e2 = 0.0;
    for (int a = 0; a < 3; ++a) {
        y[a] = scale * (R[a][0] * p[0] + R[a][1] * p[1] + R[a][2] * p[2]) + tr[a];
        const double e = y[a] - (double)g[a];
        e2 += e * e;
    }
    return sqrt(e2);
}

// From the moments and the U, V of svd3(m.K, ...): point(j, y, dist) for every point j, with its transformed coordinates y[3] and the
// distance to g's point that remains.
template <typename F>
__device__ __forceinline__ void pose_aligned_points(const float* p, const float* g, int n_pts, const PoseMoments& m, const double U[3][3],
                                                    const double V[3][3], F&& point) {
    double R[3][3], scale, tr[3];
    pose_similarity(m, U, V, R, scale, tr);
    for (int j = 0; j < n_pts; ++j) {
        double y[3], e2 = 0.0;
        for (int a = 0; a < 3; ++a) {
            y[a] = scale * (R[a][0] * p[j * 3] + R[a][1] * p[j * 3 + 1] + R[a][2] * p[j * 3 + 2]) + tr[a];
            const double e = y[a] - (double)g[j * 3 + a];
            e2 += e * e;
        }
        point(j, y, sqrt(e2));
    }
}

}  // namespace
