// Evaluation-step losses on the device: what HandMvNet._calculate_loss (handmvnet.py:279-351) computes for a root-relative
// model, the reprojection it calls (utils/camera.py:4-60 + datasets/utils.py:124-143) and the ground-truth heat maps the dataset
// builds for it (datasets/ho3d.py:155-166 -> datasets/utils.py:86-121 + Resize(antialias=True)).
//
// Conventions as in metrics.hip: sums in fp64, fixed-order reductions (LDS tree, no float atomics: bit-reproducible), and the
// per-element arithmetic the reference does in fp32 is done in fp64 -- results are compared with the reference run in float64.
//
// The target heat map is separable.  generate_heatmap stamps exp(-((x-cx)^2 + (y-cy)^2) / (2 sigma^2)) on the 6 sigma + 1 pixels
// around the truncated label (cx, cy), cropped to the image; the antialiased resize is a 1-D triangle filter per axis.  So
//   map[Y][X] = (sum_y wY[y] g(y - cy)) * (sum_x wX[x] g(x - cx)),
// two 1-D profiles of hm_w + hm_h values per joint, kept in LDS; no target tensor has to exist for the loss.
//
// Deliberate differences from the reference:
//   * a label whose whole Gaussian lies outside the image (c >= S + 3 sigma or c <= -3 sigma - 2 on either axis): the reference returns
//     a tuple (utils.py:105) and the dataset transform raises; here the map is all zero, which is what that line's comment intends;
//   * a singular extrinsic: torch.inverse raises, the kernel writes non-finite coordinates (and losses);
//   * the crop mapping scales by 256 whatever data_params["image_size"] is -- that IS the reference (handmvnet.py:332 passes no
//     image_size, datasets/utils.py:128-129 defaults to 256.), reproduced on purpose.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/handmv.h"
#include "kernels.h"
#include "pose_rows.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxProfile = 256;   // hm_h + hm_w: 21 * 256 fp64 profile values + the reduction buffer fit the 64 KB of LDS
constexpr int kMaxSigma = 8;

// Output pixel i (of n) of one axis of the target map: the cropped 1-D Gaussian around trunc(p) on S source pixels through
// the antialiased bilinear filter of torch's _upsample_bilinear2d_aa (scale = S / n; support = scale when down-sampling, else 1;
// window [int(centre - support + .5), int(centre + support + .5)) cut to [0, S); triangle weights normalised per output pixel).
__device__ double target_profile(float p, int S, int n, int sigma, int i) {
    if (!(fabsf(p) < 1.0e9f)) return 0.0;          // NaN / absurd labels: no Gaussian anywhere near the image
    const int c = (int)p;                          // astype(np.int32): toward zero (utils.py:99)
    const int r = 3 * sigma;
    const int lo = max(c - r, 0), hi = min(c + r + 1, S);   // the taps generate_heatmap keeps (utils.py:114-120)
    if (lo >= hi) return 0.0;
    const double scale = (double)S / (double)n;
    const double support = scale >= 1.0 ? scale : 1.0;
    const double invscale = scale >= 1.0 ? 1.0 / scale : 1.0;
    const double center = scale * ((double)i + 0.5);
    const int xmin = max((int)(center - support + 0.5), 0);
    const int xend = min((int)(center + support + 0.5), S);
    if (max(xmin, lo) >= min(xend, hi)) return 0.0;
    double total = 0.0;
    for (int j = xmin; j < xend; ++j) total += fmax(0.0, 1.0 - fabs(((double)j - center + 0.5) * invscale));
    const double inv2s2 = 1.0 / (2.0 * (double)sigma * (double)sigma);
    double acc = 0.0;
    for (int j = max(xmin, lo); j < min(xend, hi); ++j) {
        const double w = fmax(0.0, 1.0 - fabs(((double)j - center + 0.5) * invscale)) / total;
        const double d = (double)(j - c);
        acc += w * exp(-(d * d) * inv2s2);
    }
    return acc;
}

// prof[j][0 .. w) = column profile of joint j of this frame, prof[j][w .. w + h) = row profile.  joints: [21][2] of the frame.
__device__ void fill_profiles(const float *__restrict__ joints, int S, int h, int w, int sigma, double *prof) {
    const int per = h + w;
    for (int e = threadIdx.x; e < NJ * per; e += kThreads) {
        const int j = e / per, r = e - j * per;
        prof[e] = r < w ? target_profile(joints[j * 2 + 0], S, w, sigma, r) : target_profile(joints[j * 2 + 1], S, h, sigma, r - w);
    }
    __syncthreads();
}

// Element e of the frame's [21][h][w] target, from the profiles: one fp64 product, cast once.
__device__ __forceinline__ float target_at(const double *prof, int e, int h, int w) {
    const int hw = h * w;
    const int j = e / hw, rem = e - j * hw;
    const int y = rem / w, x = rem - y * w;
    const double *pj = prof + j * (h + w);
    return (float)(pj[w + y] * pj[x]);
}

// (a) [n][21][2] crop-image joints -> [n][21][h][w] fp32 maps; one workgroup per frame.
__global__ __launch_bounds__(kThreads) void target_heatmaps_kernel(const float *__restrict__ joints, int S, int h, int w, int sigma,
                                                                  float *__restrict__ out) {
    extern __shared__ double lds[];
    const long f = blockIdx.x;
    fill_profiles(joints + f * NJ * 2, S, h, w, sigma, lds);
    const int len = NJ * h * w;
    float *o = out + f * len;
    for (int e = threadIdx.x; e < len; e += kThreads) o[e] = target_at(lds, e, h, w);
}

// (b) get_2d_joints_from_3d_joints (project_joint, pose_rows.h), one lane per (sample, view, joint).
__global__ __launch_bounds__(kThreads) void project_joints_kernel(const float *__restrict__ joints, int B, int V, int root_idx,
                                                                 const float *__restrict__ intrinsic, const float *__restrict__ extrinsic,
                                                                 const float *__restrict__ bbox, float *__restrict__ out) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= (long)B * V * NJ) return;
    const long bv = i / NJ;
    const int j = (int)(i - bv * NJ);
    const long b = bv / V;
    double u, v;
    project_joint(joints + (b * NJ + j) * 3, nullptr, extrinsic + (b * V + root_idx) * 16, extrinsic + bv * 16, intrinsic + bv * 4,
                  bbox ? bbox + bv * 4 : nullptr, u, v);
    out[i * 2] = (float)u;
    out[i * 2 + 1] = (float)v;
}

// (c), first launch: one workgroup per frame sums (pred - target)^2 over its 21 * h * w elements into partial[frame].  target == NULL:
// the targets are rebuilt from the frame's label joints through the same target_at as (a), so both forms see the same fp32
// values.  The elements are walked in groups of four (16-byte loads where both frame bases allow, scalar loads otherwise) and
// added in the same order either way, so neither alignment nor the target form changes the bits.
// Frame slot f by its workgroup.  lds: the reduction buffer (kThreads doubles) with the profile area behind it.
__device__ __forceinline__ void frame_partial(const float *__restrict__ pred, const float *__restrict__ target,
                                              const float *__restrict__ labels, int S, int h, int w, int sigma,
                                              double *__restrict__ partial, long f, double *lds) {
    const int t = threadIdx.x;
    double *prof = lds + kThreads;
    if (!target) fill_profiles(labels + f * NJ * 2, S, h, w, sigma, prof);
    const int len = NJ * h * w;
    const float *p = pred + f * len;
    const float *g = target ? target + f * len : nullptr;
    const bool vec = ((uintptr_t)p & 15) == 0 && (!g || ((uintptr_t)g & 15) == 0);
    const int groups = (len + 3) / 4;
    double acc = 0.0;
    for (int q = t; q < groups; q += kThreads) {
        const int e0 = q * 4;
        const int cnt = min(4, len - e0);
        float pv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {0.f, 0.f, 0.f, 0.f};
        if (vec && cnt == 4) {
            const float4 a = *reinterpret_cast<const float4 *>(p + e0);
            pv[0] = a.x; pv[1] = a.y; pv[2] = a.z; pv[3] = a.w;
            if (g) {
                const float4 b = *reinterpret_cast<const float4 *>(g + e0);
                gv[0] = b.x; gv[1] = b.y; gv[2] = b.z; gv[3] = b.w;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) {
                    pv[k] = p[e0 + k];
                    if (g) gv[k] = g[e0 + k];
                }
        }
        if (!g) {   // target_at(prof, e0 + k, h, w) for the group, with the (joint, row, column) split done once
            const int hw = h * w;
            int j = e0 / hw;
            const int rem = e0 - j * hw;
            int y = rem / w, x = rem - y * w;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < cnt) {
                    const double *pj = prof + j * (h + w);
                    gv[k] = (float)(pj[w + y] * pj[x]);
                    if (++x == w) {
                        x = 0;
                        if (++y == h) { y = 0; ++j; }
                    }
                }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {   // lanes past the end hold 0 - 0
            const double d = (double)pv[k] - (double)gv[k];
            acc = fma(d, d, acc);
        }
    }
    const double s = block_sum<kThreads>(acc, lds);
    if (t == 0) partial[f] = s;
}

__global__ __launch_bounds__(kThreads) void pose_losses_kernel(const float *__restrict__ pred, const float *__restrict__ target,
                                                              const float *__restrict__ labels, int S, int h, int w, int sigma,
                                                              double *__restrict__ partial) {
    extern __shared__ double lds[];
    frame_partial(pred, target, labels, S, h, w, sigma, partial, blockIdx.x, lds);
}

// (c) for a ragged view set, first launch: the same per frame slot; the workgroup of an ABSENT slot writes partial 0 and leaves before
// it touches LDS or a barrier (the test depends on the slot only: the whole workgroup takes it), so nothing of that slot is read and
// no target map is synthesised for it.
__global__ __launch_bounds__(kThreads) void pose_losses_views_kernel(const float *__restrict__ pred, const float *__restrict__ target,
                                                                    const float *__restrict__ labels, int S, int h, int w, int sigma,
                                                                    const uint8_t *__restrict__ present, double *__restrict__ partial) {
    extern __shared__ double lds[];
    const long f = blockIdx.x;
    if (!present[f]) {
        if (threadIdx.x == 0) partial[f] = 0.0;
        return;
    }
    frame_partial(pred, target, labels, S, h, w, sigma, partial, f, lds);
}

struct FinishParams {
    const double *partial;
    const float *pred_2d, *gt_2d, *pred_cam, *gt_cam, *root_joint, *intrinsic, *extrinsic, *bbox;
    const uint8_t *mask;
    float *projected, *result;
    int B, V, hm_h, hm_w, root_idx, use_mask, with_projection;
    float w_hm, w_2d, w_3d, w_g2d, w_p2d;
};

// (c), second launch (one workgroup): the frame partials in index order, the L1 terms, the reprojection terms, the total.
//
// kRagged, a ragged view set (present: [B][V]): the value of a view-dependent term is the mean over samples of the sample's own mean
// over its v_b present views: sum_b sum_{v in P_b} x / (v_b * n) / B.  Written as
//     sum over ALL slots, in the uniform order, of (present ? x : 0) * (V / v_b),  divided by the uniform divisor B * V * n,
// so that a full mask (V / v_b == 1.0 exactly) walks through the uniform instantiation's additions and gives its bits.  An absent
// slot's rows are not read.  A sample WITHOUT a present view (a broken precondition) has V / 0 = inf, its slots add 0 * inf: the
// view-dependent terms come out NaN, and nothing is indexed by a count.
// The uniform instantiation is the same statements with every slot there and the weight the literal 1.0 (x * 1.0 is x): it tests no
// `present` and has no count array.
template <bool kRagged>
__device__ __forceinline__ void losses_finish(const FinishParams &a, const uint8_t *__restrict__ present, const int *cnt) {
    __shared__ double red[kThreads];
    const int t = threadIdx.x;
    auto there = [&](long slot) {
        if constexpr (kRagged) return present[slot] != 0;
        else return true;
    };
    auto weight = [&](long b) {
        if constexpr (kRagged) return view_weight(present, cnt, b, a.V);
        else return 1.0;
    };

    const long frames = (long)a.B * a.V;
    double s = 0.0;
    for (long i = t; i < frames; i += kThreads) s += a.partial[i] * weight(i / a.V);   // an absent slot's partial is the first launch's 0
    const double hm = block_sum<kThreads>(s, red);

    // joints_2d: masked joints are zeroed on both sides, the divisor stays the full count (models/utils.py:123-131)
    const long n2 = frames * NJ * 2;
    s = 0.0;
    for (long e = t; e < n2; e += kThreads) {
        const long bv = e / (NJ * 2);
        double d = 0.0;
        if (there(bv)) {
            const double keep = (a.use_mask && a.mask[e >> 1]) ? 0.0 : 1.0;
            d = fabs((double)a.pred_2d[e] * keep - (double)a.gt_2d[e] * keep);
        }
        s += d * weight(bv / a.V);
    }
    const double l2d = block_sum<kThreads>(s, red);

    const long n3 = (long)a.B * NJ * 3;
    s = 0.0;
    for (long e = t; e < n3; e += kThreads) s += fabs((double)a.pred_cam[e] - (double)a.gt_cam[e]);
    const double l3d = block_sum<kThreads>(s, red);

    double g2d = 0.0, p2d = 0.0;
    if (a.with_projection) {
        double sg = 0.0, sp = 0.0;
        for (long i = t; i < frames * NJ; i += kThreads) {
            const long bv = i / NJ;
            const int j = (int)(i - bv * NJ);
            const long b = bv / a.V;
            double u = 0.0, v = 0.0, dg = 0.0, dp = 0.0;
            if (there(bv)) {   // the camera tables are full [B][V]: the root camera's row is read whether or not its frame is present
                project_joint(a.pred_cam + (b * NJ + j) * 3, a.root_joint ? a.root_joint + b * 3 : nullptr,
                              a.extrinsic + (b * a.V + a.root_idx) * 16, a.extrinsic + bv * 16, a.intrinsic + bv * 4, a.bbox + bv * 4, u, v);
                dg = fabs(u - (double)a.gt_2d[i * 2]) + fabs(v - (double)a.gt_2d[i * 2 + 1]);
                dp = fabs(u - (double)a.pred_2d[i * 2]) + fabs(v - (double)a.pred_2d[i * 2 + 1]);
            }
            if (a.projected) {   // zeros for an absent slot
                a.projected[i * 2] = (float)u;
                a.projected[i * 2 + 1] = (float)v;
            }
            const double wgt = weight(b);
            sg += dg * wgt;
            sp += dp * wgt;
        }
        g2d = block_sum<kThreads>(sg, red);
        p2d = block_sum<kThreads>(sp, red);
    }
    if (t == 0) {
        const double t_hm = (double)a.w_hm * hm / ((double)frames * NJ * a.hm_h * a.hm_w);
        const double t_2d = (double)a.w_2d * l2d / (double)n2;
        const double t_3d = (double)a.w_3d * l3d / (double)n3;
        const double t_g = a.with_projection ? (double)a.w_g2d * g2d / (double)n2 : 0.0;
        const double t_p = a.with_projection ? (double)a.w_p2d * p2d / (double)n2 : 0.0;
        a.result[0] = (float)t_hm;
        a.result[1] = (float)t_2d;
        a.result[2] = (float)t_3d;
        a.result[3] = (float)t_g;
        a.result[4] = (float)t_p;
        a.result[5] = (float)(t_hm + t_2d + t_3d + t_g + t_p);   // root_3d_loss is the constant 0 of a root-relative model
    }
}

// Two kernels and not one with a nullable mask: the uniform one is the reference the tests hold the ragged one to under a full mask.
__global__ __launch_bounds__(kThreads) void pose_losses_finish_kernel(FinishParams a) { losses_finish<false>(a, nullptr, nullptr); }

__global__ __launch_bounds__(kThreads) void pose_losses_views_finish_kernel(FinishParams a, const uint8_t *__restrict__ present) {
    __shared__ int cnt[kCountSlots];
    fill_view_counts<kThreads>(cnt, present, a.B, a.V);
    __syncthreads();
    losses_finish<true>(a, present, cnt);
}

using hmv::bad_arg;
using hmv::hip_fail;

// shape rules shared by the entries that build target maps
const char *check_map_shape(int32_t image_size, int32_t hm_h, int32_t hm_w, int32_t sigma) {
    if (image_size < 1 || image_size > (1 << 20)) return "image_size must be in 1 .. 2^20";
    if (hm_h < 1 || hm_w < 1 || hm_h + hm_w > kMaxProfile) return "hm_h and hm_w must be >= 1 with hm_h + hm_w <= 256";
    if (sigma < 1 || sigma > kMaxSigma) return "sigma must be an integer in 1 .. 8";
    return nullptr;
}

}  // namespace

extern "C" int hmv_op_target_heatmaps(int32_t device, const float *joints, int32_t n_frames, int32_t image_size, int32_t hm_h,
                                      int32_t hm_w, int32_t sigma, float *out, void *stream) {
    const char *who = "hmv_op_target_heatmaps";
    if (!joints) return bad_arg(who, "joints is NULL");
    if (!out) return bad_arg(who, "out is NULL");
    if (n_frames < 1 || n_frames > (1 << 24)) return bad_arg(who, "n_frames must be in 1 .. 2^24");
    if (const char *m = check_map_shape(image_size, hm_h, hm_w, sigma)) return bad_arg(who, m);
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    const size_t lds = sizeof(double) * NJ * (size_t)(hm_h + hm_w);
    hipLaunchKernelGGL(target_heatmaps_kernel, dim3(n_frames), dim3(kThreads), lds, (hipStream_t)stream, joints, image_size, hm_h, hm_w,
                       sigma, out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}

extern "C" int hmv_project_joints(int32_t device, const float *joints_abs, int32_t B, int32_t V, int32_t root_idx,
                                  const float *intrinsic, const float *extrinsic, const float *bbox, float *out, void *stream) {
    const char *who = "hmv_project_joints";
    if (!joints_abs) return bad_arg(who, "joints_abs is NULL");
    if (!intrinsic) return bad_arg(who, "intrinsic is NULL");
    if (!extrinsic) return bad_arg(who, "extrinsic is NULL");
    if (!out) return bad_arg(who, "out is NULL");
    if (B < 1) return bad_arg(who, "B must be >= 1");
    if (V < 1) return bad_arg(who, "V must be >= 1");
    if ((int64_t)B * V > (1 << 24)) return bad_arg(who, "B * V must not exceed 2^24 frames");
    if (root_idx < 0 || root_idx >= V) return bad_arg(who, "root_idx must be in 0 .. V - 1");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    const long n = (long)B * V * NJ;
    hipLaunchKernelGGL(project_joints_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                       joints_abs, B, V, root_idx, intrinsic, extrinsic, bbox, out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}

extern "C" size_t hmv_pose_losses_scratch_bytes(int32_t B, int32_t V) {
    return B > 0 && V > 0 ? sizeof(double) * (size_t)B * (size_t)V : 0;
}

namespace {

// the argument rules of the two loss entries, in front of every HIP call; 0 or the HMV_ERR_ARG of the first broken one
int check_loss_args(const char *who, const hmv_loss_args *a, const float *result) {
    if (!a) return bad_arg(who, "args is NULL");
    if (a->struct_size != (int32_t)sizeof(hmv_loss_args)) return bad_arg(who, "struct_size does not match this library's hmv_loss_args");
    if (!result) return bad_arg(who, "result is NULL");
    if (a->B < 1) return bad_arg(who, "B must be >= 1");
    if (a->V < 1) return bad_arg(who, "V must be >= 1");
    if ((int64_t)a->B * a->V > (1 << 24)) return bad_arg(who, "B * V must not exceed 2^24 frames");
    if (!a->pred_heatmap) return bad_arg(who, "pred_heatmap is NULL");
    if (!a->pred_joints_2d) return bad_arg(who, "pred_joints_2d is NULL");
    if (!a->gt_joints_2d) return bad_arg(who, "gt_joints_2d is NULL");
    if (!a->pred_joints_cam) return bad_arg(who, "pred_joints_cam is NULL");
    if (!a->gt_joints_cam) return bad_arg(who, "gt_joints_cam is NULL");
    // image_size and sigma matter only when the targets are synthesised, but a bad value is a bug of the caller either way
    if (const char *m = check_map_shape(a->target_heatmap ? 1 : a->image_size, a->hm_h, a->hm_w, a->target_heatmap ? 1 : a->sigma))
        return bad_arg(who, m);
    if (a->with_projection) {
        if (!a->intrinsic) return bad_arg(who, "intrinsic is NULL (with_projection is set)");
        if (!a->extrinsic) return bad_arg(who, "extrinsic is NULL (with_projection is set)");
        if (!a->bbox) return bad_arg(who, "bbox is NULL (with_projection is set)");
        if (a->root_idx < 0 || a->root_idx >= a->V) return bad_arg(who, "root_idx must be in 0 .. V - 1");
    } else if (a->projected) {
        return bad_arg(who, "projected is given but with_projection is 0");
    }
    if (!a->scratch || ((uintptr_t)a->scratch & 7)) return bad_arg(who, "scratch is NULL or not 8-byte aligned");
    if (a->scratch_bytes < hmv_pose_losses_scratch_bytes(a->B, a->V))
        return bad_arg(who, "scratch_bytes is smaller than hmv_pose_losses_scratch_bytes gives for B, V");
    return HMV_OK;
}

FinishParams finish_params(const hmv_loss_args *a, float *result) {
    FinishParams f;
    f.partial = static_cast<const double *>(a->scratch);
    f.pred_2d = a->pred_joints_2d; f.gt_2d = a->gt_joints_2d; f.pred_cam = a->pred_joints_cam; f.gt_cam = a->gt_joints_cam;
    f.root_joint = a->root_joint; f.intrinsic = a->intrinsic; f.extrinsic = a->extrinsic; f.bbox = a->bbox;
    f.mask = a->joints_mask;
    f.projected = a->projected; f.result = result;
    f.B = a->B; f.V = a->V; f.hm_h = a->hm_h; f.hm_w = a->hm_w; f.root_idx = a->root_idx;
    f.use_mask = a->joints_mask && a->mask_invisible_joints;
    f.with_projection = a->with_projection != 0;
    f.w_hm = a->w_heatmap; f.w_2d = a->w_joints_2d; f.w_3d = a->w_joints_3d; f.w_g2d = a->w_g2d; f.w_p2d = a->w_p2d;
    return f;
}

}  // namespace

extern "C" int hmv_pose_losses(int32_t device, const hmv_loss_args *a, float *result, void *stream) {
    const char *who = "hmv_pose_losses";
    if (const int rc = check_loss_args(who, a, result)) return rc;
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    hipStream_t s = (hipStream_t)stream;
    double *partial = static_cast<double *>(a->scratch);
    const size_t lds = sizeof(double) * (kThreads + (a->target_heatmap ? 0 : NJ * (size_t)(a->hm_h + a->hm_w)));
    hipLaunchKernelGGL(pose_losses_kernel, dim3((unsigned)(a->B * a->V)), dim3(kThreads), lds, s, a->pred_heatmap, a->target_heatmap,
                       a->gt_joints_2d, a->image_size, a->hm_h, a->hm_w, a->sigma, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(who, e);
    hipLaunchKernelGGL(pose_losses_finish_kernel, dim3(1), dim3(kThreads), 0, s, finish_params(a, result));
    e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}

extern "C" int hmv_pose_losses_views(int32_t device, const hmv_loss_args *a, const uint8_t *view_present, float *result, void *stream) {
    const char *who = "hmv_pose_losses_views";
    if (const int rc = check_loss_args(who, a, result)) return rc;
    if (!view_present) return bad_arg(who, "view_present is NULL (hmv_pose_losses is the entry for a batch with every view)");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    hipStream_t s = (hipStream_t)stream;
    double *partial = static_cast<double *>(a->scratch);
    const size_t lds = sizeof(double) * (kThreads + (a->target_heatmap ? 0 : NJ * (size_t)(a->hm_h + a->hm_w)));
    hipLaunchKernelGGL(pose_losses_views_kernel, dim3((unsigned)(a->B * a->V)), dim3(kThreads), lds, s, a->pred_heatmap, a->target_heatmap,
                       a->gt_joints_2d, a->image_size, a->hm_h, a->hm_w, a->sigma, view_present, partial);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(who, e);
    hipLaunchKernelGGL(pose_losses_views_finish_kernel, dim3(1), dim3(kThreads), 0, s, finish_params(a, result), view_present);
    e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}
