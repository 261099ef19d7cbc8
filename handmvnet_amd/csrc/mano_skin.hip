// MANO linear blend skinning (include/handmv.h "MANO skinning"): 16 rotation matrices and 10 shape coefficients to the mesh and the
// 21 joints, what ManoLayer.forward does with root_rot_mode = joint_rot_mode = "rotmat", use_pca=False and no th_trans / center_idx.
//   hmv_op_mano_pack   one launch per parameter set: the caller's arrays in MANO's own layouts into one kernel-layout buffer
//   hmv_op_mano_skin   one launch per call: projection of the rotations, shape and pose blend, the kinematic chain, the blend of
//                      the 16 transforms, optionally the un-alignment of hmv_op_hand_ik, millimetres, one rounding to fp32
// Arithmetic is fp64 from the fp32 inputs, every operation rounded on its own (contract(off) below).
//
// The packed buffer (hmv_mano_pack_bytes; kHeadDoubles, kHeadInts and the four float planes below are its whole layout):
//   double  JT[16][3]          J_regressor . v_template
//   double  JS[16][3][10]      J_regressor . shapedirs         (no skin launch touches the regressor)
//   int32   tips[5], n_verts, 0, 0
//   float   vt[3][Nv]          v_template, coordinate-major
//   float   sd[10][3][Nv]      shapedirs, basis-major
//   float   pd[135][3][Nv]     posedirs, basis-major: lane v of a wave reads consecutive floats of one (basis, coordinate) plane
//   float   w[16][Nv]          weights, joint-major
//
// The skin kernel is one workgroup of kTile threads per row.  A row's status is an OR over all of its vertices, and with no atomics
// that OR needs one owner, so a workgroup walks the row's vertex tiles itself instead of sharing them with others.  Lanes 0..15
// project one rotation each (svd3 of pose_rows.h), regress their joint from the folded regressor and walk their own path of the
// chain from the root (at most four links; a lane repeats its ancestors' products in their order, so G[parent] has the same bits
// on every lane that needs it); the 16 skinning transforms, the joint positions and the 135 pose-map values go to LDS.  Then one
// thread per vertex does its 3 x 145 multiply-adds and the 16-term blend.  Vector stores in plain C++; no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/handmv.h"
#include "kernels.h"

#pragma clang fp contract(off)
#include "pose_rows.h"

namespace {

constexpr int kTile = 512;         // threads of a workgroup = vertices of a tile
constexpr int kPackThreads = 256;
constexpr int kJoints = 16, kBetas = 10, kPose = 135;
constexpr int kHeadDoubles = kJoints * 3 + kJoints * 3 * kBetas;   // JT, JS
constexpr int kHeadInts = 8;                                       // tips[5], n_verts, 0, 0
constexpr int kPlanes = 3 + kBetas * 3 + kPose * 3 + kJoints;      // float planes of Nv values each
constexpr int kMaxVerts = 1 << 20;

struct Packed {
    const double *JT, *JS;
    const int *ints;
    const float *vt, *sd, *pd, *w;
};

__host__ __device__ inline Packed packed_view(const void *buf, int nv) {
    Packed p;
    p.JT = (const double *)buf;
    p.JS = p.JT + kJoints * 3;
    p.ints = (const int *)(p.JT + kHeadDoubles);
    p.vt = (const float *)(p.ints + kHeadInts);
    p.sd = p.vt + (size_t)3 * nv;
    p.pd = p.sd + (size_t)kBetas * 3 * nv;
    p.w = p.pd + (size_t)kPose * 3 * nv;
    return p;
}

struct PackTips {
    int v[5];
};

// One thread per value of the packed buffer: the first kHeadDoubles threads sum a regressor row over the vertices in ascending order
// (one-off, so the serial sum is what keeps it deterministic), the next kHeadInts write the integers, the rest transpose one float.
__global__ __launch_bounds__(kPackThreads) void mano_pack_kernel(const float *__restrict__ v_template, const float *__restrict__ shapedirs,
                                                               const float *__restrict__ posedirs, const float *__restrict__ J_regressor,
                                                               const float *__restrict__ weights, PackTips tips, int nv, void *packed) {
    const Packed pk = packed_view(packed, nv);
    const size_t total = (size_t)kHeadDoubles + kHeadInts + (size_t)kPlanes * nv;
    size_t i = (size_t)blockIdx.x * kPackThreads + threadIdx.x;
    if (i >= total) return;
    if (i < (size_t)kHeadDoubles) {
        const int idx = (int)i;
        double s = 0.0;
        if (idx < kJoints * 3) {   // JT[k][c]
            const int k = idx / 3, c = idx % 3;
            for (int v = 0; v < nv; ++v) s += (double)J_regressor[(size_t)k * nv + v] * (double)v_template[(size_t)v * 3 + c];
        } else {                   // JS[k][c][b]
            const int r = idx - kJoints * 3;
            const int k = r / (3 * kBetas), c = (r / kBetas) % 3, b = r % kBetas;
            for (int v = 0; v < nv; ++v)
                s += (double)J_regressor[(size_t)k * nv + v] * (double)shapedirs[((size_t)v * 3 + c) * kBetas + b];
        }
        ((double *)packed)[idx] = s;
        return;
    }
    i -= kHeadDoubles;
    if (i < (size_t)kHeadInts) {
        int val = 0;
        for (int f = 0; f < 5; ++f) val = (int)i == f ? tips.v[f] : val;
        val = (int)i == 5 ? nv : val;
        ((int *)pk.ints)[i] = val;
        return;
    }
    i -= kHeadInts;
    const int plane = (int)(i / (size_t)nv), v = (int)(i % (size_t)nv);
    float val;
    if (plane < 3) {
        val = v_template[(size_t)v * 3 + plane];
    } else if (plane < 3 + kBetas * 3) {
        const int q = plane - 3, b = q / 3, c = q % 3;
        val = shapedirs[((size_t)v * 3 + c) * kBetas + b];
    } else if (plane < 3 + kBetas * 3 + kPose * 3) {
        const int q = plane - 3 - kBetas * 3, p = q / 3, c = q % 3;
        val = posedirs[((size_t)v * 3 + c) * kPose + p];
    } else {
        const int k = plane - 3 - kBetas * 3 - kPose * 3;
        val = weights[(size_t)v * kJoints + k];
    }
    ((float *)pk.vt)[i] = val;
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN and inf

// Q = U V^T of the SVD of m (row-major), column 2 negated when det Q < 0: the polar factor made a rotation.
__device__ void project_rotation(double m[3][3]) {
    double U[3][3], S[3], V[3][3], Q[3][3];
    svd3(m, U, S, V);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Q[i][j] = (U[i][0] * V[j][0] + U[i][1] * V[j][1]) + U[i][2] * V[j][2];
    const bool flip = det3(Q) < 0;
    for (int i = 0; i < 3; ++i) {
        m[i][0] = Q[i][0];
        m[i][1] = Q[i][1];
        m[i][2] = flip ? -Q[i][2] : Q[i][2];
    }
}

struct SkinShared {
    double R[kJoints][9];    // the (projected) rotations
    double J[kJoints][3];    // the regressed joints of the shaped template
    double A[kJoints][12];   // the skinning transforms, rows of [R | t]
    double Gt[kJoints][3];   // the posed joints
    double pm[kPose];        // vec(R[1..15] - I)
    double beta[kBetas];
    int bad[kTile / 64];
};

// Vertex v of the row in metres: shape blend, pose blend, the 16-term blend of the transforms, applied.
__device__ __forceinline__ void skin_vertex(const Packed &pk, int nv, int v, const SkinShared &sh, double out[3]) {
    double x[3];
    for (int c = 0; c < 3; ++c) x[c] = (double)pk.vt[(size_t)c * nv + v];
    for (int b = 0; b < kBetas; ++b) {
        const double be = sh.beta[b];
        for (int c = 0; c < 3; ++c) x[c] += (double)pk.sd[(size_t)(b * 3 + c) * nv + v] * be;
    }
#pragma unroll 5
    for (int p = 0; p < kPose; ++p) {
        const double m = sh.pm[p];
        for (int c = 0; c < 3; ++c) x[c] += (double)pk.pd[(size_t)(p * 3 + c) * nv + v] * m;
    }
    double T[12];
    for (int i = 0; i < 12; ++i) T[i] = 0.0;
#pragma unroll 1   // (unrolled, the 192 doubles of A are hoisted out of the vertex loop into registers and spill)
    for (int k = 0; k < kJoints; ++k) {
        const double wk = (double)pk.w[(size_t)k * nv + v];
        for (int i = 0; i < 12; ++i) T[i] += wk * sh.A[k][i];
    }
    for (int c = 0; c < 3; ++c) out[c] = ((T[c * 4] * x[0] + T[c * 4 + 1] * x[1]) + T[c * 4 + 2] * x[2]) + T[c * 4 + 3];
}

// Metres to millimetres, then R^T (x - t) of the alignment when there is one; rounded once.
__device__ __forceinline__ void finish_point(const double m[3], const double *al, float r[3]) {
    double x[3] = {m[0] * 1000.0, m[1] * 1000.0, m[2] * 1000.0};
    if (al) {
        const double d[3] = {x[0] - al[9], x[1] - al[10], x[2] - al[11]};
        for (int c = 0; c < 3; ++c) x[c] = (al[c] * d[0] + al[3 + c] * d[1]) + al[6 + c] * d[2];
    }
    for (int c = 0; c < 3; ++c) r[c] = (float)x[c];
}

__global__ __launch_bounds__(kTile) void mano_skin_kernel(hmv_mano_skin_args a) {
    __shared__ SkinShared sh;
    const int t = (int)threadIdx.x;
    const long row = (long)blockIdx.x;
    const int nv = a.n_verts;
    const Packed pk = packed_view(a.packed, nv);
    const double *al = a.align ? a.align + row * 12 : nullptr;
    float *out_v = a.vertices ? a.vertices + row * (long)nv * 3 : nullptr;
    float *out_j = a.joints ? a.joints + row * (NJ * 3) : nullptr;

    if (pk.ints[5] != nv) {   // a buffer packed for another n_verts: nothing of it is read; the row is NaN and says so
        const float nan = __builtin_nanf("");
        if (out_v)
            for (int v = t; v < nv; v += kTile)
                for (int c = 0; c < 3; ++c) out_v[(long)v * 3 + c] = nan;
        if (out_j && t < NJ)
            for (int c = 0; c < 3; ++c) out_j[t * 3 + c] = nan;
        if (t == 0) a.status[row] = 1;
        return;   // (the same for the whole workgroup)
    }

    // ---- lanes 0..15: rotation k, joint k
    if (t < kBetas) {
        const float *be = a.betas_mode == HMV_MANO_BETAS_PER_ROW ? a.betas + row * kBetas : a.betas;
        sh.beta[t] = a.betas_mode == HMV_MANO_BETAS_NONE ? 0.0 : (double)be[t];
    }
    if (t < kJoints) {
        const float *r = a.rot + (row * kJoints + t) * 9;
        double m[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) m[i][j] = (double)r[i * 3 + j];
        if (a.project) project_rotation(m);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                sh.R[t][i * 3 + j] = m[i][j];
                if (t > 0) sh.pm[(t - 1) * 9 + i * 3 + j] = m[i][j] - (i == j ? 1.0 : 0.0);
            }
    }
    __syncthreads();
    if (t < kJoints) {
        for (int c = 0; c < 3; ++c) {
            double j = pk.JT[t * 3 + c];
            for (int b = 0; b < kBetas; ++b) j += pk.JS[(t * 3 + c) * kBetas + b] * sh.beta[b];
            sh.J[t][c] = j;
        }
    }
    __syncthreads();
    // ---- the chain: G[0] = [R0 | J0], G[k] = G[parent] [Rk | Jk - Jparent]; joint k > 0 is link (k - 1) % 3 of finger (k - 1) / 3
    if (t < kJoints) {
        const int first = t > 0 ? ((t - 1) / 3) * 3 + 1 : 0, depth = t > 0 ? t - first + 1 : 0;
        double G[3][3], g[3];
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) G[i][j] = sh.R[0][i * 3 + j];
            g[i] = sh.J[0][i];
        }
        for (int s = 1; s <= 3; ++s) {
            if (s > depth) break;
            const int k = first + s - 1, pa = s == 1 ? 0 : k - 1;
            double d[3], N[3][3];
            for (int c = 0; c < 3; ++c) d[c] = sh.J[k][c] - sh.J[pa][c];
            for (int i = 0; i < 3; ++i) g[i] = ((G[i][0] * d[0] + G[i][1] * d[1]) + G[i][2] * d[2]) + g[i];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) N[i][j] = (G[i][0] * sh.R[k][j] + G[i][1] * sh.R[k][3 + j]) + G[i][2] * sh.R[k][6 + j];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) G[i][j] = N[i][j];
        }
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 3; ++j) sh.A[t][i * 4 + j] = G[i][j];
            sh.A[t][i * 4 + 3] = g[i] - ((G[i][0] * sh.J[t][0] + G[i][1] * sh.J[t][1]) + G[i][2] * sh.J[t][2]);
            sh.Gt[t][i] = g[i];
        }
    }
    __syncthreads();

    // ---- one thread per vertex, tile after tile; the five tip vertices of the joints follow the mesh as items nv .. nv + 4 of the same
    // loop (one copy of the vertex arithmetic), computed whether or not the joints are stored, as the status covers them
    bool bad = false;
#pragma unroll 1
    for (int i = out_v ? t : nv + t; i < nv + 5; i += kTile) {
        const bool is_tip = i >= nv;
        int v = i;
        if (is_tip) {
            v = pk.ints[i - nv];
            v = v < 0 ? 0 : v >= nv ? nv - 1 : v;   // (pack refused a tip outside [0, n_verts); the clamp guards the load)
        }
        double m[3];
        float r[3];
        skin_vertex(pk, nv, v, sh, m);
        finish_point(m, al, r);
        // joint 4 f + 4 is the tip of finger f
        float *dst = is_tip ? (out_j ? out_j + (4 * (i - nv) + 4) * 3 : nullptr) : out_v + (long)v * 3;
        for (int c = 0; c < 3; ++c) {
            if (dst) dst[c] = r[c];
            bad |= !finite_f(r[c]);
        }
    }
    // ---- the other 16 joints are the chain's translations: sources [0, 13,14,15,-, 1,2,3,-, 4,5,6,-, 10,11,12,-, 7,8,9,-]
    if (t < NJ && (t == 0 || t % 4 != 0)) {
        const int f = t > 0 ? (t - 1) / 4 : 0, l = t > 0 ? (t - 1) % 4 : 0;
        const int base = f == 0 ? 13 : f == 1 ? 1 : f == 2 ? 4 : f == 3 ? 10 : 7;
        const int k = t == 0 ? 0 : base + l;
        const double m[3] = {sh.Gt[k][0], sh.Gt[k][1], sh.Gt[k][2]};
        float r[3];
        finish_point(m, al, r);
        for (int c = 0; c < 3; ++c) {
            if (out_j) out_j[t * 3 + c] = r[c];
            bad |= !finite_f(r[c]);
        }
    }
    // ---- status: the OR over the workgroup, one wave's ballot per LDS slot
    const bool wave_bad = __ballot(bad) != 0ull;
    if (t % 64 == 0) sh.bad[t / 64] = wave_bad ? 1 : 0;
    __syncthreads();
    if (t == 0) {
        int any = 0;
        for (int i = 0; i < kTile / 64; ++i) any |= sh.bad[i];
        a.status[row] = any;
    }
}

using hmv::bad_arg;
using hmv::hip_fail;

}  // namespace

extern "C" size_t hmv_mano_pack_bytes(int32_t n_verts) {
    if (n_verts <= 0 || n_verts > kMaxVerts) return 0;
    return (size_t)kHeadDoubles * sizeof(double) + (size_t)kHeadInts * sizeof(int32_t) + (size_t)kPlanes * n_verts * sizeof(float);
}

extern "C" int hmv_op_mano_pack(int32_t device, const hmv_mano_params *p, void *packed, void *stream) {
    const char *who = "hmv_op_mano_pack";
    if (!p) return bad_arg(who, "params is NULL");
    if (p->struct_size != (int32_t)sizeof(hmv_mano_params)) return bad_arg(who, "struct_size does not match this library's hmv_mano_params");
    if (p->n_verts <= 0 || p->n_verts > kMaxVerts) return bad_arg(who, "n_verts must be in 1 .. 2^20");
    if (!p->v_template) return bad_arg(who, "v_template is NULL");
    if (!p->shapedirs) return bad_arg(who, "shapedirs is NULL");
    if (!p->posedirs) return bad_arg(who, "posedirs is NULL");
    if (!p->J_regressor) return bad_arg(who, "J_regressor is NULL");
    if (!p->weights) return bad_arg(who, "weights is NULL");
    for (int f = 0; f < 5; ++f)
        if (p->tips[f] < 0 || p->tips[f] >= p->n_verts) return bad_arg(who, "tips holds a vertex index outside [0, n_verts)");
    if (!packed || ((uintptr_t)packed & 7)) return bad_arg(who, "packed is NULL or not 8-byte aligned");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    PackTips tips;
    for (int f = 0; f < 5; ++f) tips.v[f] = p->tips[f];
    const size_t total = (size_t)kHeadDoubles + kHeadInts + (size_t)kPlanes * p->n_verts;
    const unsigned blocks = (unsigned)((total + kPackThreads - 1) / kPackThreads);
    hipLaunchKernelGGL(mano_pack_kernel, dim3(blocks), dim3(kPackThreads), 0, (hipStream_t)stream, p->v_template, p->shapedirs, p->posedirs,
                       p->J_regressor, p->weights, tips, p->n_verts, packed);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}

extern "C" int hmv_op_mano_skin(int32_t device, const hmv_mano_skin_args *a, void *stream) {
    const char *who = "hmv_op_mano_skin";
    if (!a) return bad_arg(who, "args is NULL");
    if (a->struct_size != (int32_t)sizeof(hmv_mano_skin_args)) return bad_arg(who, "struct_size does not match this library's hmv_mano_skin_args");
    if (a->n <= 0) return bad_arg(who, "n must be positive");
    if (a->n_verts <= 0 || a->n_verts > kMaxVerts) return bad_arg(who, "n_verts must be in 1 .. 2^20");
    if (!a->packed || ((uintptr_t)a->packed & 7)) return bad_arg(who, "packed is NULL or not 8-byte aligned");
    if (!a->rot) return bad_arg(who, "rot is NULL");
    if (a->betas_mode != HMV_MANO_BETAS_NONE && a->betas_mode != HMV_MANO_BETAS_SHARED && a->betas_mode != HMV_MANO_BETAS_PER_ROW)
        return bad_arg(who, "betas_mode must be 0 (none), 1 (shared) or 2 (per_row)");
    if (a->betas_mode != HMV_MANO_BETAS_NONE && !a->betas) return bad_arg(who, "betas is NULL although betas_mode asks for it");
    if (a->align && ((uintptr_t)a->align & 7)) return bad_arg(who, "align is not 8-byte aligned");
    if (!a->vertices && !a->joints) return bad_arg(who, "vertices and joints are both NULL");
    if (!a->status) return bad_arg(who, "status is NULL");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    hipLaunchKernelGGL(mano_skin_kernel, dim3((unsigned)a->n), dim3(kTile), 0, (hipStream_t)stream, *a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}
