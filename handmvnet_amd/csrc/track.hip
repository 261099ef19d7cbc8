// Following the hand through a sequence: the crop window of frame t + 1 is the box around the hand found in frame t.
// Reproduces, per frame slot (sample, view),
//   batch_cropped_joints_to_joints_img  (datasets/utils.py:146-162, as handmvnet.py:237 calls it: torch fp32)
//   points2d_to_bbox                    (datasets/utils.py:5-27)
// on the device, so that hmv_forward_frames' windows (int32) and bbox (fp32) can be updated in place between two time steps with
// nothing on the host (include/handmv.h: hmv_op_next_crop_boxes, hmv_forward_frames_track, hmv_forward_frames_views_track).
//
// One wave64 per row of 21 joints, four rows per workgroup.  Lanes 0..20 hold a joint each (the lanes above repeat joint 20, which
// leaves minimum and maximum alone); min / max travel across the wave with shuffles: no LDS, no atomics.  Every lane reads the row's
// window before any lane writes it, and no row reads another row's window, so the outputs may alias the inputs.
//
// The second kernel closes the loop through space: the windows of ALL cameras of a sample from one 3D pose (the triangulated joints, or
// the model's root-relative pose on the triangulated root), which is
//   get_2d_joints_from_3d_joints        (utils/camera.py:25-44; project_joint, pose_rows.h)
//   points2d_to_bbox                    (the same window_of as above)
// per (sample, view) in the same shape: one wave64 per slot, a joint per lane (include/handmv.h: hmv_op_reproject_crop_boxes).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/handmv.h"
#include "kernels.h"
#include "pose_rows.h"   // (NJ, project_joint; included in front of the contract(off) below: its arithmetic keeps losses.hip's bits)

namespace {

constexpr int kWave = 64;
constexpr int kRowsPerBlock = 4;
constexpr long long kMaxWindow = 1 << 16;   // what the frame preparation still takes for a window (misc_kernels.hip)
constexpr float kMaxCoord = 1e9f;           // beyond it int conversion would overflow: the reference raises, the kernel reports
constexpr int kMaxViews = 16;               // hmv_op_triangulate's

// hipcc contracts a * b + c into one fma by default, and one fused rounding can move an integer box edge.  The __fmul_rn /
// __fadd_rn of the HIP headers are plain operators compiled with contraction allowed, so they fuse once inlined; the helpers below,
// and the kernel that inlines them, are compiled without.
#pragma clang fp contract(off)
__device__ __forceinline__ float mul_rn(float x, float y) { return x * y; }
__device__ __forceinline__ float add_rn(float x, float y) { return x + y; }
__device__ __forceinline__ float sub_rn(float x, float y) { return x - y; }
__device__ __forceinline__ float div_rn(float x, float y) { return x / y; }   // (fp32 division is correctly rounded by default)

__device__ __forceinline__ float wave_min(float v) {
    for (int m = kWave / 2; m >= 1; m >>= 1) v = fminf(v, __shfl_xor(v, m, kWave));
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
    for (int m = kWave / 2; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, kWave));
    return v;
}

__device__ __forceinline__ double wave_sum(double v) {   // fixed order: the same tree whatever the call holds
    for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// points2d_to_bbox (datasets/utils.py:5-27) of the wave's points, one (X, Y) per lane, every lane of the wave calling: int() of the float
// minimum / maximum truncates toward zero, the shorter side of a `square` box is widened by |h - w| (the odd pixel goes to the low
// edge), then the margin.  False, and `out` left alone, for a window wider or taller than kMaxWindow.  The points are finite and below
// kMaxCoord (the caller's check), so every edge fits an int: |edge| < 1e9 + 2^16.
__device__ __forceinline__ bool window_of(float X, float Y, int margin, int square, int out[4]) {
    long long x_min = (long long)(int)wave_min(X), y_min = (long long)(int)wave_min(Y);
    long long x_max = (long long)(int)wave_max(X), y_max = (long long)(int)wave_max(Y);
    const long long w = x_max - x_min, h = y_max - y_min;
    if (square && h != w) {
        const long long diff = h > w ? h - w : w - h, pad = diff / 2, lead = (diff % 2 == 0) ? pad : pad + 1;
        if (h > w) { x_min -= lead; x_max += pad; }
        else       { y_min -= lead; y_max += pad; }
    }
    const long long m = margin;
    x_min -= m; y_min -= m; x_max += m; y_max += m;
    if (x_max - x_min <= kMaxWindow && y_max - y_min <= kMaxWindow) {
        out[0] = (int)x_min; out[1] = (int)y_min; out[2] = (int)x_max; out[3] = (int)y_max;
        return true;
    }
    return false;
}

__global__ __launch_bounds__(kWave * kRowsPerBlock) void next_crop_boxes_kernel(hmv::TrackParams a) {
    const int lane = (int)threadIdx.x % kWave;
    const long row = (long)blockIdx.x * kRowsPerBlock + (int)threadIdx.x / kWave;
    if (row >= a.n_rows) return;   // (wave-uniform)
    const long slot = a.index ? (long)a.index[row] : row;
    if (slot < 0 || slot >= a.n_slots) return;   // the forward reads such a frame as the black view; there is no window to move

    int box[4];
    for (int i = 0; i < 4; ++i) box[i] = a.boxes_in[slot * 4 + i];
    int out[4] = {box[0], box[1], box[2], box[3]};
    int st;

    if (a.present && !a.present[slot]) {
        st = 1;
        if (a.joints_img && lane < NJ * 2) a.joints_img[slot * (NJ * 2) + lane] = 0.f;
    } else {
        // batch_cropped_joints_to_joints_img in its own operation order, every operation rounded on its own (no contraction to an fma)
        const int j = lane < NJ ? lane : NJ - 1;
        const float u = a.joints_crop_img[row * (NJ * 2) + j * 2], v = a.joints_crop_img[row * (NJ * 2) + j * 2 + 1];
        const float S = (float)a.image_size;
        const float x1f = (float)box[0], y1f = (float)box[1];
        const float wf = sub_rn((float)box[2], x1f), hf = sub_rn((float)box[3], y1f);
        const float X = add_rn(mul_rn(u, div_rn(wf, S)), x1f);
        const float Y = add_rn(mul_rn(v, div_rn(hf, S)), y1f);
        if (a.joints_img && lane < NJ) {
            a.joints_img[slot * (NJ * 2) + lane * 2] = X;
            a.joints_img[slot * (NJ * 2) + lane * 2 + 1] = Y;
        }
        const bool bad = !(fabsf(X) < kMaxCoord) || !(fabsf(Y) < kMaxCoord);   // NaN and inf included
        const bool any_bad = __ballot(bad) != 0ull;
        st = 2;
        if (!any_bad) {
            if (window_of(X, Y, a.margin, a.square, out)) st = 0;
        }
    }
    if (lane < 4) {
        const int e = lane == 0 ? out[0] : lane == 1 ? out[1] : lane == 2 ? out[2] : out[3];
        a.boxes_out[slot * 4 + lane] = e;
        if (a.bbox_out) a.bbox_out[row * 4 + lane] = (float)e;
    }
    if (a.status && lane == 0) a.status[slot] = st;
}

// One wave64 per slot (sample b, view v): lanes 0..20 project a joint each (the lanes above repeat joint 20).  Nothing a slot reads is
// written by the launch but its own status, which every lane reads before lane 0 writes it.
__global__ __launch_bounds__(kWave * kRowsPerBlock) void reproject_crop_boxes_kernel(hmv_reproject_boxes_args a) {
    const int lane = (int)threadIdx.x % kWave;
    const long slot = (long)blockIdx.x * kRowsPerBlock + (int)threadIdx.x / kWave;
    if (slot >= (long)a.B * a.V) return;   // (wave-uniform)
    const long b = slot / a.V;
    const int j = lane < NJ ? lane : NJ - 1;
    const float nan = __builtin_nanf("");

    // the sample rule: 63 finite coordinates, a frame camera among the views, a triangulated root (or every joint)
    const float *x3 = a.points3d + (b * NJ + j) * 3;
    const bool finite = isfinite(x3[0]) && isfinite(x3[1]) && isfinite(x3[2]);
    const int fc = a.frame_cam ? a.frame_cam[b] : 0;
    bool ok = __ballot(!finite) == 0ull && fc >= 0 && fc < a.V;
    if (a.point_status) {
        if (a.require_all) ok = ok && __ballot(a.point_status[b * NJ + j] != 0) == 0ull;
        else ok = ok && a.point_status[b * NJ] == 0;
    }
    if (!ok) {
        if (a.joints_reproj && lane < NJ * 2) a.joints_reproj[slot * (NJ * 2) + lane] = nan;
        if (lane == 0) {
            a.source[slot] = 0;
            if (a.gap) a.gap[slot] = nan;
        }
        return;
    }

    double u, v, z;
    project_joint(x3, nullptr, a.extrinsic + (b * a.V + fc) * 16, a.extrinsic + slot * 16, a.intrinsic + slot * 4, nullptr, u, v, &z);
    const float X = (float)u, Y = (float)v;   // fp64 from the fp32 inputs, rounded once
    if (a.joints_reproj && lane < NJ) {
        a.joints_reproj[slot * (NJ * 2) + lane * 2] = X;
        a.joints_reproj[slot * (NJ * 2) + lane * 2 + 1] = Y;
    }
    const int st_in = a.status[slot];
    if (a.gap) {   // the mean distance of the view's own 2D joints from the reprojection, of the fp32 values as written
        float g = nan;
        if (a.joints_img && st_in == 0) {   // (wave-uniform)
            const double dx = (double)a.joints_img[slot * (NJ * 2) + j * 2] - (double)X;
            const double dy = (double)a.joints_img[slot * (NJ * 2) + j * 2 + 1] - (double)Y;
            g = (float)(wave_sum(lane < NJ ? sqrt(dx * dx + dy * dy) : 0.0) / (double)NJ);
        }
        if (lane == 0) a.gap[slot] = g;
    }

    // the slot rule: every joint in front of the camera, finite and below kMaxCoord, a window within kMaxWindow
    const bool bad = !(z > 0.0) || !isfinite(u) || !isfinite(v) || !(fabsf(X) < kMaxCoord) || !(fabsf(Y) < kMaxCoord);
    int out[4] = {0, 0, 0, 0};
    const bool moved = __ballot(bad) == 0ull && window_of(X, Y, a.margin, a.square, out);
    if (moved && lane < 4) {
        const int e = lane == 0 ? out[0] : lane == 1 ? out[1] : lane == 2 ? out[2] : out[3];
        a.crop_boxes[slot * 4 + lane] = e;
        if (a.bbox) a.bbox[slot * 4 + lane] = (float)e;
    }
    if (lane == 0) {
        a.source[slot] = moved ? 1 : 0;
        if (moved && st_in == 2) a.status[slot] = 0;   // a kept window that moved after all; an absent view (1) stays absent
    }
}

using hmv::bad_arg;
using hmv::hip_fail;

}  // namespace

namespace hmv {

hipError_t launch_next_crop_boxes(const TrackParams &p, hipStream_t s) {
    const unsigned blocks = (unsigned)((p.n_rows + kRowsPerBlock - 1) / kRowsPerBlock);
    hipLaunchKernelGGL(next_crop_boxes_kernel, dim3(blocks), dim3(kWave * kRowsPerBlock), 0, s, p);
    return hipGetLastError();
}

}  // namespace hmv

extern "C" int hmv_op_next_crop_boxes(int32_t device, int32_t n_slots, const float *joints_crop_img, const int32_t *crop_boxes_in,
                                      const uint8_t *present, int32_t image_size, int32_t margin, int32_t square, int32_t *crop_boxes_out,
                                      float *bbox_out, float *joints_img, int32_t *status, void *stream) {
    const char *who = "hmv_op_next_crop_boxes";
    if (n_slots <= 0) return bad_arg(who, "n_slots must be positive");
    if (image_size <= 0) return bad_arg(who, "image_size must be positive");
    if (margin < 0) return bad_arg(who, "margin must not be negative");
    if (!joints_crop_img || !crop_boxes_in || !crop_boxes_out) return bad_arg(who, "joints_crop_img, crop_boxes_in and crop_boxes_out are required");
    if (hipSetDevice(device) != hipSuccess) { hmv::set_thread_error(std::string(who) + ": hipSetDevice failed"); return HMV_ERR_HIP; }
    hmv::TrackParams p{n_slots, n_slots, joints_crop_img, crop_boxes_in, present, nullptr, image_size, margin, square != 0,
                       crop_boxes_out, bbox_out, joints_img, status};
    const hipError_t e = hmv::launch_next_crop_boxes(p, static_cast<hipStream_t>(stream));
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}

extern "C" int hmv_op_reproject_crop_boxes(int32_t device, const hmv_reproject_boxes_args *a, void *stream) {
    const char *who = "hmv_op_reproject_crop_boxes";
    if (!a) return bad_arg(who, "args is NULL");
    if (a->struct_size < (int32_t)sizeof(hmv_reproject_boxes_args))
        return bad_arg(who, "struct_size is smaller than this library's hmv_reproject_boxes_args");
    if (a->B < 1) return bad_arg(who, "B must be >= 1");
    if (a->V < 1 || a->V > kMaxViews) return bad_arg(who, "V must be in 1 .. 16");
    if ((int64_t)a->B * a->V > (1 << 24)) return bad_arg(who, "B * V must not exceed 2^24 frames");
    if (a->margin < 0) return bad_arg(who, "margin must not be negative");
    if (!a->points3d) return bad_arg(who, "points3d is NULL");
    if (!a->intrinsic) return bad_arg(who, "intrinsic is NULL");
    if (!a->extrinsic) return bad_arg(who, "extrinsic is NULL");
    if (!a->crop_boxes) return bad_arg(who, "crop_boxes is NULL");
    if (!a->status) return bad_arg(who, "status is NULL");
    if (!a->source) return bad_arg(who, "source is NULL");
    if (hipSetDevice(device) != hipSuccess) { hmv::set_thread_error(std::string(who) + ": hipSetDevice failed"); return HMV_ERR_HIP; }
    const unsigned blocks = (unsigned)(((long)a->B * a->V + kRowsPerBlock - 1) / kRowsPerBlock);
    hipLaunchKernelGGL(reproject_crop_boxes_kernel, dim3(blocks), dim3(kWave * kRowsPerBlock), 0, static_cast<hipStream_t>(stream), *a);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}
