// Hand pose parameters from 21 joints (include/handmv.h "hand IK"): everything JointsToVertices.__call__ (models/joints_to_vertices.py:25-50)
// does around its MANO layer, per sample, on the device:
//   hmv_op_hand_ik        the three-point rigid alignment onto the template (utils/misc.py:10-47 as joints_to_vertices.py:27-39 calls it)
//                         and the analytic inverse kinematics adaptive_IK (utils/analytical_ik.py:50-138): 16 rotation matrices
//   hmv_op_rigid_unapply  the inverse of that alignment on the layer's vertices (joints_to_vertices.py:48)
// Arithmetic is fp64 from the fp32 inputs in the reference's operation order, every operation rounded on its own.
//
// hand_ik is shaped like track.hip: one wave64 per sample, four samples per workgroup.  Lanes 0..20 hold a joint each.  The two 3x3
// SVDs (alignment, global rotation) run on lane 0 and their results travel to the wave by shuffles; once R0 is known the five fingers
// are independent, and lanes 0..4 walk the three joints of one finger each (every lane runs the same instructions on a clamped
// finger index, so no shuffle sits under a branch).  No LDS, no atomics; vector stores in plain C++.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/handmv.h"
#include "kernels.h"

// No a * b + c is contracted into an fma anywhere below, svd3 included: "the reference's operation order" then means something.
#pragma clang fp contract(off)
#include "pose_rows.h"

namespace {

constexpr int kWave = 64;
constexpr int kRowsPerBlock = 4;
constexpr int kUnapplyThreads = 256;

__device__ __forceinline__ double bcast(double v, int src) { return __shfl(v, src, kWave); }

// a = v u^T of two 3x3 matrices held by columns of singular vectors: r[i][j] = sum_k v[i][k] u[j][k]
#define IK_V_UT(r, v, u)                                                                                                          \
    for (int i = 0; i < 3; ++i)                                                                                                   \
        for (int j = 0; j < 3; ++j) r[i][j] = v[i][0] * u[j][0] + v[i][1] * u[j][1] + v[i][2] * u[j][2];

// rigid_transform_3D (misc.py:23-45) of three points: a[k][c], b[k][c] are point k of the prediction / of the template.
// H has rank 2, so the third singular vectors carry an arbitrary sign: the determinant rule alone makes R the proper rotation.
__device__ __forceinline__ void align_three(const double a[3][3], const double b[3][3], double R[3][3], double t[3]) {
    double ca[3], cb[3];
    for (int c = 0; c < 3; ++c) {
        ca[c] = ((a[0][c] + a[1][c]) + a[2][c]) / 3.0;
        cb[c] = ((b[0][c] + b[1][c]) + b[2][c]) / 3.0;
    }
    double H[3][3];   // Am @ Bm.T
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            H[i][j] = ((a[0][i] - ca[i]) * (b[0][j] - cb[j]) + (a[1][i] - ca[i]) * (b[1][j] - cb[j])) + (a[2][i] - ca[i]) * (b[2][j] - cb[j]);
    double U[3][3], S[3], V[3][3];
    svd3(H, U, S, V);
    IK_V_UT(R, V, U)
    if (det3(R) < 0) {   // Vt[2, :] *= -1
        for (int i = 0; i < 3; ++i) V[i][2] = -V[i][2];
        IK_V_UT(R, V, U)
    }
    for (int i = 0; i < 3; ++i) t[i] = -((R[i][0] * ca[0] + R[i][1] * ca[1]) + R[i][2] * ca[2]) + cb[i];
}

// R0 of adaptive_IK (analytical_ik.py:80-99): tp[k][c], pp[k][c] are palm vector k (joints 1, 5, 9, 13, 17 minus joint 0) of the
// template / of the aligned joints.  The reference's own reflection rule: V's last column changes sign only when det R0 is -1 AND a
// singular value is (absolutely) below 1e-4 -- a mirrored hand with a non-planar palm keeps its reflection.
__device__ __forceinline__ void global_rotation(const double tp[5][3], const double pp[5][3], double R0[3][3]) {
    double H[3][3];   // T_0 @ P_0.T
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double h = tp[0][i] * pp[0][j];
            for (int k = 1; k < 5; ++k) h += tp[k][i] * pp[k][j];
            H[i][j] = h;
        }
    double U[3][3], S[3], V[3][3];
    svd3(H, U, S, V);
    IK_V_UT(R0, V, U)
    if (fabs(det3(R0) + 1.0) < 1e-6 && (fabs(S[0]) < 1e-4 || fabs(S[1]) < 1e-4 || fabs(S[2]) < 1e-4)) {
        for (int i = 0; i < 3; ++i) V[i][2] = -V[i][2];
        IK_V_UT(R0, V, U)
    }
}

// transforms3d.axangles.axangle2mat(axis, angle, is_normalized=False) with c = cos(angle), s = sin(angle) given: the axis is divided
// by its norm (once more, for the swing axis), then the Rodrigues matrix in that function's operation order.
__device__ __forceinline__ void axangle(const double ax[3], double c, double s, double D[3][3]) {
    const double n = sqrt((ax[0] * ax[0] + ax[1] * ax[1]) + ax[2] * ax[2]);
    const double x = ax[0] / n, y = ax[1] / n, z = ax[2] / n;
    const double C = 1.0 - c;
    const double xs = x * s, ys = y * s, zs = z * s;
    const double xC = x * C, yC = y * C, zC = z * C;
    const double xyC = x * yC, yzC = y * zC, zxC = z * xC;
    D[0][0] = x * xC + c; D[0][1] = xyC - zs;   D[0][2] = zxC + ys;
    D[1][0] = xyC + zs;   D[1][1] = y * yC + c; D[1][2] = yzC - xs;
    D[2][0] = zxC - ys;   D[2][1] = yzC + xs;   D[2][2] = z * zC + c;
}

// One step of the chain (analytical_ik.py:112-130) for joint k with parent pa: on entry R = R[pa] and q = q[pa_pa]; bone_pa = T[pa] -
// T[pa_pa], bone_k = T[k] - T[pa], pk = P[k].  Leaves R = R[k], q = q[pa] and the local rotation R_pa_k in D.
// R[pa] is R0 times Rodrigues matrices, orthogonal by construction (a reflection R0 included), so its inverse is its transpose.
__device__ __forceinline__ void chain_step(double R[3][3], double q[3], const double bone_pa[3], const double bone_k[3], const double pk[3],
                                           double D[3][3]) {
    double d[3], dp[3];
    for (int i = 0; i < 3; ++i) {
        q[i] = ((R[i][0] * bone_pa[0] + R[i][1] * bone_pa[1]) + R[i][2] * bone_pa[2]) + q[i];
    }
    for (int i = 0; i < 3; ++i) d[i] = pk[i] - q[i];
    for (int i = 0; i < 3; ++i) dp[i] = (R[0][i] * d[0] + R[1][i] * d[1]) + R[2][i] * d[2];
    const double *dt = bone_k;
    double ta[3] = {dt[1] * dp[2] - dt[2] * dp[1], dt[2] * dp[0] - dt[0] * dp[2], dt[0] * dp[1] - dt[1] * dp[0]};
    const double na = sqrt((ta[0] * ta[0] + ta[1] * ta[1]) + ta[2] * ta[2]) + 1e-8;
    for (int i = 0; i < 3; ++i) ta[i] = ta[i] / na;
    const double nt = sqrt((dt[0] * dt[0] + dt[1] * dt[1]) + dt[2] * dt[2]) + 1e-8;
    const double np_ = sqrt((dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2]) + 1e-8;
    const double cos_alpha = ((dt[0] * dp[0] + dt[1] * dp[1]) + dt[2] * dp[2]) / (nt * np_);
    const double alpha = acos(cos_alpha);   // unclamped: a cosine above 1 is NaN here as there
    double Dsw[3][3], Dtw[3][3];
    axangle(ta, cos(alpha), sin(alpha), Dsw);
    axangle(dt, 1.0, 0.0, Dtw);             // angle 0 about the template bone: the identity for any non-zero bone
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) D[i][j] = (Dsw[i][0] * Dtw[0][j] + Dsw[i][1] * Dtw[1][j]) + Dsw[i][2] * Dtw[2][j];
    double Rk[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rk[i][j] = (R[i][0] * D[0][j] + R[i][1] * D[1][j]) + R[i][2] * D[2][j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = Rk[i][j];
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN and inf

__global__ __launch_bounds__(kWave * kRowsPerBlock) void hand_ik_kernel(hmv::HandIkParams a) {
    const int lane = (int)threadIdx.x % kWave;
    const long row = (long)blockIdx.x * kRowsPerBlock + (int)threadIdx.x / kWave;
    if (row >= a.n) return;   // (wave-uniform)
    const float *J = a.joints + row * (NJ * 3);
    const float *T = a.tmpl;
    const int j = lane < NJ ? lane : NJ - 1;   // the lanes above repeat joint 20 and store nothing
    const double p[3] = {(double)J[j * 3], (double)J[j * 3 + 1], (double)J[j * 3 + 2]};

    // ---- alignment of joints 0, 9, 13 onto the template's: lane 0, then 12 shuffles
    double Ra[3][3], ta[3];
    if (lane == 0) {
        double pa[3][3], pb[3][3];
        for (int c = 0; c < 3; ++c) {
            pa[0][c] = (double)J[c];  pa[1][c] = (double)J[9 * 3 + c];  pa[2][c] = (double)J[13 * 3 + c];
            pb[0][c] = (double)T[c];  pb[1][c] = (double)T[9 * 3 + c];  pb[2][c] = (double)T[13 * 3 + c];
        }
        align_three(pa, pb, Ra, ta);
    } else {
        for (int i = 0; i < 3; ++i) {
            Ra[i][0] = Ra[i][1] = Ra[i][2] = 0.0;
            ta[i] = 0.0;
        }
    }
    for (int i = 0; i < 3; ++i) {
        for (int c = 0; c < 3; ++c) Ra[i][c] = bcast(Ra[i][c], 0);
        ta[i] = bcast(ta[i], 0);
    }
    // joints_to_mano = (ret_R @ joints.T + ret_t).T, one joint per lane, kept in fp64 for the IK as the reference keeps it
    double P[3];
    for (int i = 0; i < 3; ++i) P[i] = ((Ra[i][0] * p[0] + Ra[i][1] * p[1]) + Ra[i][2] * p[2]) + ta[i];

    // ---- global rotation from the five palm vectors: gathered to every lane by shuffles, solved on lane 0, 9 shuffles back
    double pp[5][3], tp[5][3];
    {
        double P0[3];
        for (int c = 0; c < 3; ++c) P0[c] = bcast(P[c], 0);
        for (int k = 0; k < 5; ++k)
            for (int c = 0; c < 3; ++c) {
                pp[k][c] = bcast(P[c], 1 + 4 * k) - P0[c];
                tp[k][c] = (double)T[(1 + 4 * k) * 3 + c] - (double)T[c];
            }
    }
    double R[3][3];
    if (lane == 0) {
        global_rotation(tp, pp, R);
    } else {
        for (int i = 0; i < 3; ++i) R[i][0] = R[i][1] = R[i][2] = 0.0;
    }
    for (int i = 0; i < 3; ++i)
        for (int c = 0; c < 3; ++c) R[i][c] = bcast(R[i][c], 0);

    bool bad = false;
    float *out_R = a.pose_R + row * (16 * 9);
    if (lane == 0)
        for (int i = 0; i < 9; ++i) {
            const float v = (float)R[i / 3][i % 3];
            out_R[i] = v;   // slot 0 = R[0]
            bad |= !finite_f(v);
        }

    // ---- the chain: finger f = joints 4f + 1 .. 4f + 4 on lane f; R[4f + 1] = R0, q[0] = T[0]
    const int f = lane < 5 ? lane : 4;
    const int base = 1 + 4 * f;
    double q[3] = {(double)T[0], (double)T[1], (double)T[2]};
    double bone_pa[3];
    for (int c = 0; c < 3; ++c) bone_pa[c] = (double)T[base * 3 + c] - (double)T[c];
    // ID2ROT (analytical_ik.py:32-38): the fingers' first slots are 13, 1, 4, 10, 7 and a finger's three slots are consecutive
    const int slot = f == 0 ? 13 : f == 1 ? 1 : f == 2 ? 4 : f == 3 ? 10 : 7;
    for (int s = 0; s < 3; ++s) {
        const int k = base + 1 + s;
        double pk[3], bone_k[3], D[3][3];
        for (int c = 0; c < 3; ++c) {
            pk[c] = __shfl(P[c], k, kWave);
            bone_k[c] = (double)T[k * 3 + c] - (double)T[(k - 1) * 3 + c];
        }
        chain_step(R, q, bone_pa, bone_k, pk, D);
        for (int c = 0; c < 3; ++c) bone_pa[c] = bone_k[c];
        if (lane < 5)
            for (int i = 0; i < 9; ++i) {
                const float v = (float)D[i / 3][i % 3];
                out_R[(slot + s) * 9 + i] = v;   // slot ID2ROT[k] = R_pa_k[k]
                bad |= !finite_f(v);
            }
    }

    if (lane < 12) {   // ret_R row-major, then ret_t, as fp64
        double v = ta[0];
        for (int i = 0; i < 3; ++i)
            for (int c = 0; c < 3; ++c) v = lane == i * 3 + c ? Ra[i][c] : v;
        v = lane == 10 ? ta[1] : lane == 11 ? ta[2] : v;
        a.align[row * 12 + lane] = v;
        bad |= !(fabs(v) <= 1.7976931348623157e308);
    }
    if (lane < NJ)
        for (int c = 0; c < 3; ++c) {
            const float v = (float)P[c];
            if (a.aligned) a.aligned[row * (NJ * 3) + lane * 3 + c] = v;
            bad |= !finite_f(v);
        }
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0) a.status[row] = any_bad ? 1 : 0;
}

// out = R^T (p - t): np.linalg.inv(ret_R) @ (mano_v.T - ret_t) with the inverse of a rotation as its transpose.  One thread per
// point; a thread reads its point before it writes it and no thread reads another's, so out may be points.
__global__ __launch_bounds__(kUnapplyThreads) void rigid_unapply_kernel(const float *points, const double *__restrict__ align, long total, int n_pts,
                                                                      float *out) {
    const long i = (long)blockIdx.x * kUnapplyThreads + (int)threadIdx.x;
    if (i >= total) return;
    const double *A = align + (i / n_pts) * 12;
    const double d[3] = {(double)points[i * 3] - A[9], (double)points[i * 3 + 1] - A[10], (double)points[i * 3 + 2] - A[11]};
    float r[3];
    for (int c = 0; c < 3; ++c) r[c] = (float)((A[c] * d[0] + A[3 + c] * d[1]) + A[6 + c] * d[2]);
    for (int c = 0; c < 3; ++c) out[i * 3 + c] = r[c];
}

using hmv::bad_arg;
using hmv::hip_fail;

}  // namespace

namespace hmv {

hipError_t launch_hand_ik(const HandIkParams &p, hipStream_t s) {
    const unsigned blocks = (unsigned)((p.n + kRowsPerBlock - 1) / kRowsPerBlock);
    hipLaunchKernelGGL(hand_ik_kernel, dim3(blocks), dim3(kWave * kRowsPerBlock), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_rigid_unapply(const float *points, const double *align, long n, int n_pts, float *out, hipStream_t s) {
    const long total = n * n_pts;
    const unsigned blocks = (unsigned)((total + kUnapplyThreads - 1) / kUnapplyThreads);
    hipLaunchKernelGGL(rigid_unapply_kernel, dim3(blocks), dim3(kUnapplyThreads), 0, s, points, align, total, n_pts, out);
    return hipGetLastError();
}

}  // namespace hmv

extern "C" int hmv_op_hand_ik(int32_t device, const float *joints, const float *template_joints, int32_t n, float *pose_R, double *align,
                              float *joints_aligned, int32_t *status, void *stream) {
    const char *who = "hmv_op_hand_ik";
    if (n <= 0) return bad_arg(who, "n must be positive");
    if (!joints) return bad_arg(who, "joints is NULL");
    if (!template_joints) return bad_arg(who, "template_joints is NULL");
    if (!pose_R) return bad_arg(who, "pose_R is NULL");
    if (!align || ((uintptr_t)align & 7)) return bad_arg(who, "align is NULL or not 8-byte aligned");
    if (!status) return bad_arg(who, "status is NULL");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    const hmv::HandIkParams p{joints, template_joints, (long)n, pose_R, align, joints_aligned, status};
    const hipError_t e = hmv::launch_hand_ik(p, (hipStream_t)stream);
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}

extern "C" int hmv_op_rigid_unapply(int32_t device, const float *points, const double *align, int32_t n, int32_t n_pts, float *out,
                                    void *stream) {
    const char *who = "hmv_op_rigid_unapply";
    if (n <= 0) return bad_arg(who, "n must be positive");
    if (n_pts <= 0) return bad_arg(who, "n_pts must be positive");
    if (!points) return bad_arg(who, "points is NULL");
    if (!align || ((uintptr_t)align & 7)) return bad_arg(who, "align is NULL or not 8-byte aligned");
    if (!out) return bad_arg(who, "out is NULL");
    if (((long)n * n_pts + kUnapplyThreads - 1) / kUnapplyThreads > 0x7fffffffL) return bad_arg(who, "n * n_pts is too large for one launch");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    const hipError_t e = hmv::launch_rigid_unapply(points, align, (long)n, n_pts, out, (hipStream_t)stream);
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}
