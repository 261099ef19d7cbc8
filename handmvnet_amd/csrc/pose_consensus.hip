// Pose consensus over reference views (include/handmv.h "pose consensus"): S estimates of the same hand, estimate s root-relative in
// the frame of camera ref_cam[s] (a reference-view sweep, hmv_forward_orders), rotated into ONE camera's frame by the extrinsics,
// then their mean or geometric median per joint, the per-joint disagreement and each estimate's distance from the consensus.
//
// The rotation is utils/camera.py:4-22 (transform_joints_between_cameras: world = E_src [x; 1], target = inverse(E_tgt) world) applied
// to a root-relative pose, T(x) - T(0): only the 3x3 part of inverse(E_tgt) E_src acts, no translation.
//
// Arithmetic is fp64 from the fp32 inputs, every operation rounded on its own, in the order handmv.h documents and
// tests/consensus_oracle.py repeats; outputs are rounded once to fp32.
//
// Shaped like hand_ik.hip and track.hip: one wave64 per sample, four samples per workgroup.  Lanes 0..20 hold one joint each and loop
// over the estimates; every lane of a live wave runs the same instructions on a clamped joint index, so the shuffles of the
// per-estimate joint sum sit under no branch.  No LDS, no atomics; vector stores in plain C++; rows beyond B exit as whole waves.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/handmv.h"
#include "kernels.h"

// No a * b + c is contracted into an fma anywhere below, solve4_xyz included.
#pragma clang fp contract(off)
#include "pose_rows.h"

namespace {

constexpr int kWave = 64;
constexpr int kRowsPerBlock = 4;

// y = M[:3, :3] x with M = inverse(E_tgt) E_src: M[r][c] = ((T[r][0] E[0][c] + T[r][1] E[1][c]) + T[r][2] E[2][c]) + T[r][3] E[3][c],
// y[r] = (M[r][0] x[0] + M[r][1] x[1]) + M[r][2] x[2].  bad: the estimate's ref_cam was out of range -- NaN.
__device__ __forceinline__ void align_point(const double T[3][4], const float *__restrict__ e_src, const float *__restrict__ x, bool bad,
                                            double y[3]) {
    const double x0 = (double)x[0], x1 = (double)x[1], x2 = (double)x[2];
    for (int r = 0; r < 3; ++r) {
        double m[3];
        for (int c = 0; c < 3; ++c)
            m[c] = ((T[r][0] * (double)e_src[c] + T[r][1] * (double)e_src[4 + c]) + T[r][2] * (double)e_src[8 + c]) + T[r][3] * (double)e_src[12 + c];
        y[r] = (m[0] * x0 + m[1] * x1) + m[2] * x2;
        if (bad) y[r] = (double)NAN;
    }
}

__device__ __forceinline__ double dist2(const double a[3], const double b[3]) {
    const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
    return (d0 * d0 + d1 * d1) + d2 * d2;
}

__global__ __launch_bounds__(kWave * kRowsPerBlock) void pose_consensus_kernel(const hmv::PoseConsensusParams p) {
    const int lane = (int)threadIdx.x & (kWave - 1);
    const long b = (long)blockIdx.x * kRowsPerBlock + ((int)threadIdx.x >> 6);
    if (b >= p.B) return;   // (a whole wave)
    const int j = lane < NJ ? lane : NJ - 1;
    const bool live = lane < NJ;
    const int S = p.S, V = p.V;
    const float *ext = p.extrinsic + b * V * 16;
    double T[3][4];
    inverse_rows(ext + (long)p.target * 16, T);

    // estimate s of this lane's joint in the target frame
    auto estimate = [&](int s, double x[3]) {
        const int rc = p.ref_cam[s];
        const bool bad = rc < 0 || rc >= V;
        const int cam = rc < 0 ? 0 : (rc >= V ? V - 1 : rc);
        align_point(T, ext + (long)cam * 16, p.poses + (((long)s * p.B + b) * NJ + j) * 3, bad, x);
    };

    // the mean, summed over s ascending; the aligned rows leave here
    double y[3] = {0.0, 0.0, 0.0};
    for (int s = 0; s < S; ++s) {
        double x[3];
        estimate(s, x);
        for (int c = 0; c < 3; ++c) y[c] += x[c];
        if (p.aligned && live) {
            float *o = p.aligned + (((long)s * p.B + b) * NJ + j) * 3;
            const float o0 = (float)x[0], o1 = (float)x[1], o2 = (float)x[2];
            o[0] = o0; o[1] = o1; o[2] = o2;
        }
    }
    for (int c = 0; c < 3; ++c) y[c] /= (double)S;

    // the geometric median: Weiszfeld steps from the mean, exactly p.iterations of them
    if (p.mode == 1)
        for (int it = 0; it < p.iterations; ++it) {
            double num[3] = {0.0, 0.0, 0.0}, den = 0.0;
            for (int s = 0; s < S; ++s) {
                double x[3];
                estimate(s, x);
                const double d = fmax(sqrt(dist2(x, y)), 1e-12);
                for (int c = 0; c < 3; ++c) num[c] += x[c] / d;
                den += 1.0 / d;
            }
            for (int c = 0; c < 3; ++c) y[c] = num[c] / den;
        }
    if (p.consensus && live) {
        float *o = p.consensus + (b * NJ + j) * 3;
        const float o0 = (float)y[0], o1 = (float)y[1], o2 = (float)y[2];
        o[0] = o0; o[1] = o1; o[2] = o2;
    }
    if (!p.spread && !p.deviation) return;   // (the same for the whole grid)

    // spread: sqrt(sum_s |x_s - y|^2 / S) per joint; deviation: per estimate the joints' |x_s - y| summed in joint order, / 21
    double sq = 0.0;
    for (int s = 0; s < S; ++s) {
        double x[3];
        estimate(s, x);
        const double d2 = dist2(x, y);
        sq += d2;
        const double d = sqrt(d2);
        double sum = 0.0;
        for (int k = 0; k < NJ; ++k) sum += __shfl(d, k, kWave);
        if (p.deviation && lane == 0) p.deviation[(long)s * p.B + b] = (float)(sum / (double)NJ);
    }
    if (p.spread && live) p.spread[b * NJ + j] = (float)sqrt(sq / (double)S);
}

using hmv::bad_arg;
using hmv::hip_fail;

}  // namespace

namespace hmv {

hipError_t launch_pose_consensus(const PoseConsensusParams &p, hipStream_t s) {
    const unsigned blocks = (unsigned)((p.B + kRowsPerBlock - 1) / kRowsPerBlock);
    hipLaunchKernelGGL(pose_consensus_kernel, dim3(blocks), dim3(kWave * kRowsPerBlock), 0, s, p);
    return hipGetLastError();
}

}  // namespace hmv

extern "C" int hmv_op_pose_consensus(int32_t device, const hmv_consensus_args *a, void *stream) {
    const char *who = "hmv_op_pose_consensus";
    if (!a) return bad_arg(who, "args is NULL");
    if (a->struct_size != (int32_t)sizeof(hmv_consensus_args)) return bad_arg(who, "struct_size does not match this library's hmv_consensus_args");
    if (a->S < 1) return bad_arg(who, "S must be >= 1");
    if (a->B < 1) return bad_arg(who, "B must be >= 1");
    if (a->V < 1) return bad_arg(who, "V must be >= 1");
    if (a->target_cam < 0 || a->target_cam >= a->V) return bad_arg(who, "target_cam is outside [0, V)");
    if (a->mode != 0 && a->mode != 1) return bad_arg(who, "mode must be 0 (mean) or 1 (geometric median)");
    if (a->iterations < 0) return bad_arg(who, "iterations must not be negative");
    if (!a->poses) return bad_arg(who, "poses is NULL");
    if (!a->ref_cam) return bad_arg(who, "ref_cam is NULL");
    if (!a->extrinsic) return bad_arg(who, "extrinsic is NULL");
    if (!a->aligned && !a->consensus && !a->spread && !a->deviation) return bad_arg(who, "every output is NULL");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    const hmv::PoseConsensusParams p{a->poses, a->ref_cam, a->extrinsic, a->S, a->B, a->V, a->target_cam, a->mode, a->iterations,
                                     a->aligned, a->consensus, a->spread, a->deviation};
    const hipError_t e = hmv::launch_pose_consensus(p, (hipStream_t)stream);
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}
