// Evaluating a followed sequence on the device (include/handmv.h "sequence evaluation"): three stateless entries.
//   hmv_op_labels_to_windows  frame-space label joints into the windows a step ran on: batch_joints_img_to_cropped_joints
//                             (datasets/utils.py:124-143) to the bits of the reference's fp32 torch run, plus per slot how many visible
//                             label joints fell outside the window
//   hmv_op_mka                PoseMetrics.mka (models/metrics.py:36-49): mean keypoint acceleration of [B][T][n_pts][dim], in fp64
//   hmv_seq_eval_add          one time step of B concurrent sequences ("lanes") into caller-owned running sums: jitter of predictions and
//                             labels from a two-step history, the tracker's status counts, the window-quality counts of the first entry
//
// The mapping is shaped like track.hip: one wave64 per slot, four slots per workgroup, lanes 0..20 hold a joint each, counts travel by
// ballot: no LDS, no atomics.  mka is one workgroup per sequence with a fixed-order LDS tree; the accumulation is one wave per lane
// with a fixed-order shuffle tree and a final read-modify-write of the sums by one thread per element in plain C++.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/handmv.h"
#include "kernels.h"

namespace {

constexpr int NJ = 21;
constexpr int kWave = 64;
constexpr int kRowsPerBlock = 4;
constexpr int kMkaThreads = 256;
constexpr int kSums = 12;              // doubles per lane (layout: include/handmv.h)
constexpr int kPose = NJ * 3;          // floats of one pose
constexpr int kHistory = 2 * 2 * kPose;   // floats per lane: {predictions, labels} x {step t - 2, step t - 1} x 63

// Every operation below is rounded on its own: hipcc would otherwise contract a * b + c into one fma (see track.hip), and one fused
// rounding moves a label by an ulp (the mapping) or changes the stated operation order (the accelerations).
#pragma clang fp contract(off)
__device__ __forceinline__ float mul_rn(float x, float y) { return x * y; }
__device__ __forceinline__ float sub_rn(float x, float y) { return x - y; }
__device__ __forceinline__ float div_rn(float x, float y) { return x / y; }   // (fp32 division is correctly rounded by default)

struct LabelParams {
    int n_slots, image_size;
    const float *joints_img;
    const int *boxes;
    const uint8_t *present, *mask_in;
    float *joints_crop;
    uint8_t *mask_out;
    int *slot_info;
};

__global__ __launch_bounds__(kWave * kRowsPerBlock) void labels_to_windows_kernel(LabelParams a) {
    const int lane = (int)threadIdx.x % kWave;
    const long slot = (long)blockIdx.x * kRowsPerBlock + (int)threadIdx.x / kWave;
    if (slot >= a.n_slots) return;   // (wave-uniform)

    const int x1 = a.boxes[slot * 4], y1 = a.boxes[slot * 4 + 1], x2 = a.boxes[slot * 4 + 2], y2 = a.boxes[slot * 4 + 3];
    const int st = (a.present && !a.present[slot]) ? 1 : (x2 <= x1 || y2 <= y1) ? 2 : 0;
    const bool joint = lane < NJ;
    const bool hidden = joint && a.mask_in && a.mask_in[slot * NJ + lane] != 0;

    const float S = (float)a.image_size;
    float u = 0.f, v = 0.f;
    if (st == 0 && joint) {
        // pts -= (x1, y1);  pts[..., 0] *= image_size / widths: torch evaluates a Python scalar over a tensor as reciprocal() * scalar
        const float x1f = (float)x1, y1f = (float)y1;
        const float wf = sub_rn((float)x2, x1f), hf = sub_rn((float)y2, y1f);
        const float X = a.joints_img[slot * (NJ * 2) + lane * 2], Y = a.joints_img[slot * (NJ * 2) + lane * 2 + 1];
        u = mul_rn(sub_rn(X, x1f), mul_rn(div_rn(1.f, wf), S));
        v = mul_rn(sub_rn(Y, y1f), mul_rn(div_rn(1.f, hf), S));
    }
    const bool seen = st == 0 && joint && !hidden;
    const bool out = seen && !(u >= 0.f && u < S && v >= 0.f && v < S);   // NaN and inf count as outside
    const int visible = __popcll(__ballot(seen)), outside = __popcll(__ballot(out));

    if (joint) {
        a.joints_crop[slot * (NJ * 2) + lane * 2] = u;
        a.joints_crop[slot * (NJ * 2) + lane * 2 + 1] = v;
        if (a.mask_out) a.mask_out[slot * NJ + lane] = (hidden || st != 0) ? 1 : 0;
    }
    if (a.slot_info && lane < 3) a.slot_info[slot * 3 + lane] = lane == 0 ? st : lane == 1 ? outside : visible;
}

// ||(p0 + p2) - 2 p1|| of one keypoint in fp64 from fp32 inputs, in the reference's operation order (metrics.py:47-49)
__device__ __forceinline__ double acc_norm(const float *p0, const float *p1, const float *p2, int dim) {
    double ss = 0.0;
    for (int d = 0; d < dim; ++d) {
        const double acc = ((double)p0[d] + (double)p2[d]) - 2.0 * (double)p1[d];
        ss += acc * acc;
    }
    return sqrt(ss);
}

__global__ __launch_bounds__(kMkaThreads) void mka_kernel(const float *__restrict__ preds, int T, int n_pts, int dim, float *__restrict__ out) {
    __shared__ double red[kMkaThreads];
    const int t = (int)threadIdx.x;
    const long rows = T >= 3 ? (long)(T - 2) * n_pts : 0;   // acceleration rows of one sequence
    const long step = (long)n_pts * dim;
    const float *seq = preds + (long)blockIdx.x * T * step;
    double sum = 0.0;
    for (long r = t; r < rows; r += kMkaThreads) {   // row r = (time r / n_pts, keypoint r % n_pts): the same offset in three consecutive steps
        const float *p = seq + r * dim;
        sum += acc_norm(p, p + step, p + 2 * step, dim);
    }
    red[t] = sum;
    __syncthreads();
    for (int s = kMkaThreads / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    if (t == 0) out[blockIdx.x] = rows > 0 ? (float)(red[0] / (double)rows) : nanf("");   // the mean of an empty tensor
}

struct SeqParams {
    const float *pred, *gt;
    const int *track_status, *slot_info;
    const uint8_t *restart;
    double *sums;
    float *history;
    int V;
};

__device__ __forceinline__ double wave_sum(double v) {
    for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);   // IEEE addition commutes: every lane ends with the same bits
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
    for (int m = kWave / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// One wave per lane b of the batch.  Lanes 0..20 of the wave hold a keypoint each.
__global__ __launch_bounds__(kWave) void seq_eval_add_kernel(SeqParams a) {
    const int lane = (int)threadIdx.x;
    const long b = blockIdx.x;
    double *sums = a.sums + b * kSums;
    float *hist = a.history + b * kHistory;
    const double since = (a.restart && a.restart[b]) ? 1.0 : sums[0] + 1.0;   // steps since the restart, this one included
    const bool full = since >= 3.0;                                           // the history holds the two previous steps of this sequence

    double acc_p = 0.0, acc_g = 0.0;
    if (lane < NJ) {
        for (int w = 0; w < (a.gt ? 2 : 1); ++w) {
            const float *cur = (w == 0 ? a.pred : a.gt) + b * kPose + lane * 3;
            float *h0 = hist + (w * 2) * kPose + lane * 3, *h1 = h0 + kPose;
            const float c[3] = {cur[0], cur[1], cur[2]};
            if (full) (w == 0 ? acc_p : acc_g) = acc_norm(h0, h1, c, 3);
            for (int d = 0; d < 3; ++d) {   // read above, written here: the newer step becomes the older one
                h0[d] = h1[d];
                h1[d] = c[d];
            }
        }
    }
    acc_p = wave_sum(acc_p);
    acc_g = wave_sum(acc_g);

    int n_st[3] = {0, 0, 0}, n_empty = 0, n_vis = 0, n_out = 0;
    for (int v = lane; v < a.V; v += kWave) {
        if (a.track_status) {
            const int s = a.track_status[b * a.V + v];
            n_st[0] += s == 0; n_st[1] += s == 1; n_st[2] += s == 2;
        }
        if (a.slot_info) {
            const int *si = a.slot_info + (b * a.V + v) * 3;
            n_empty += si[0] == 2; n_out += si[1]; n_vis += si[2];
        }
    }
    for (int i = 0; i < 3; ++i) n_st[i] = wave_sum(n_st[i]);
    n_empty = wave_sum(n_empty); n_vis = wave_sum(n_vis); n_out = wave_sum(n_out);

    if (lane < kSums) {   // one thread per element: plain load, plain store
        const double old = sums[lane];
        double now = old;
        switch (lane) {
            case 0: now = since; break;
            case 1: now = old + 1.0; break;
            case 2: now = old + (full ? (double)NJ : 0.0); break;
            case 3: now = old + acc_p; break;
            case 4: now = a.gt ? old + acc_g : old; break;
            case 5: case 6: case 7: now = old + (double)n_st[lane - 5]; break;
            case 8: now = old + (double)n_empty; break;
            case 9: now = old + (double)n_vis; break;
            case 10: now = old + (double)n_out; break;
            default: break;
        }
        sums[lane] = now;
    }
}

using hmv::bad_arg;
using hmv::hip_fail;

}  // namespace

extern "C" int hmv_op_labels_to_windows(int32_t device, int32_t n_slots, const float *joints_img, const int32_t *crop_boxes,
                                        const uint8_t *present, const uint8_t *joints_mask_in, int32_t image_size, float *joints_crop,
                                        uint8_t *mask_out, int32_t *slot_info, void *stream) {
    const char *who = "hmv_op_labels_to_windows";
    if (n_slots <= 0) return bad_arg(who, "n_slots must be positive");
    if (image_size <= 0) return bad_arg(who, "image_size must be positive");
    if (!joints_img) return bad_arg(who, "joints_img is NULL");
    if (!crop_boxes) return bad_arg(who, "crop_boxes is NULL");
    if (!joints_crop) return bad_arg(who, "joints_crop is NULL");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    const LabelParams p{n_slots, image_size, joints_img, crop_boxes, present, joints_mask_in, joints_crop, mask_out, slot_info};
    const unsigned blocks = (unsigned)(((long)n_slots + kRowsPerBlock - 1) / kRowsPerBlock);
    hipLaunchKernelGGL(labels_to_windows_kernel, dim3(blocks), dim3(kWave * kRowsPerBlock), 0, (hipStream_t)stream, p);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}

extern "C" int hmv_op_mka(int32_t device, const float *preds, int32_t B, int32_t T, int32_t n_pts, int32_t dim, float *out, void *stream) {
    const char *who = "hmv_op_mka";
    if (B <= 0) return bad_arg(who, "B must be positive");
    if (T < 0) return bad_arg(who, "T must not be negative");
    if (n_pts <= 0) return bad_arg(who, "n_pts must be positive");
    if (dim < 1 || dim > 4) return bad_arg(who, "dim must be in 1 .. 4");
    if (!preds) return bad_arg(who, "preds is NULL");
    if (!out) return bad_arg(who, "out is NULL");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    hipLaunchKernelGGL(mka_kernel, dim3((unsigned)B), dim3(kMkaThreads), 0, (hipStream_t)stream, preds, T, n_pts, dim, out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}

extern "C" size_t hmv_seq_eval_sums_doubles(int32_t B) { return B >= 1 ? (size_t)B * kSums : 0; }

extern "C" size_t hmv_seq_eval_history_floats(int32_t B) { return B >= 1 ? (size_t)B * kHistory : 0; }

extern "C" int hmv_seq_eval_add(int32_t device, const hmv_seq_eval_args *a, void *stream) {
    const char *who = "hmv_seq_eval_add";
    if (!a) return bad_arg(who, "args is NULL");
    if (a->struct_size != (int32_t)sizeof(hmv_seq_eval_args)) return bad_arg(who, "struct_size does not match this library's hmv_seq_eval_args");
    if (a->B < 1) return bad_arg(who, "B must be >= 1");
    if (a->V < 1) return bad_arg(who, "V must be >= 1");
    if ((int64_t)a->B * a->V > (1 << 24)) return bad_arg(who, "B * V must not exceed 2^24 frames");
    if (!a->pred_joints_cam) return bad_arg(who, "pred_joints_cam is NULL");
    if (!a->sums || ((uintptr_t)a->sums & 7)) return bad_arg(who, "sums is NULL or not 8-byte aligned");
    if (!a->history || ((uintptr_t)a->history & 3)) return bad_arg(who, "history is NULL or not 4-byte aligned");
    if (a->sums_doubles < hmv_seq_eval_sums_doubles(a->B)) return bad_arg(who, "sums_doubles is smaller than hmv_seq_eval_sums_doubles gives for B");
    if (a->history_floats < hmv_seq_eval_history_floats(a->B))
        return bad_arg(who, "history_floats is smaller than hmv_seq_eval_history_floats gives for B");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    const SeqParams p{a->pred_joints_cam, a->gt_joints_cam, a->track_status, a->slot_info, a->restart, a->sums, a->history, a->V};
    hipLaunchKernelGGL(seq_eval_add_kernel, dim3((unsigned)a->B), dim3(kWave), 0, (hipStream_t)stream, p);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}
