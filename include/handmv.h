/*
 * handmv.h -- C ABI of libhandmv.so, the MI355X-native (gfx950) HandMvNet inference engine.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference has no FFI
 * layer of its own; the boundary it exposes is the Python object protocol of
 *   HandMvNet(train_params, model_params, data_params)      /root/reference/src/models/handmvnet.py:28
 *   HandMvNet.forward(x, bbox=None, cam_params=None)->dict  /root/reference/src/models/handmvnet.py:158-266
 *   load_state_dict(state_dict, strict=True)                /root/reference/src/eval.py:46,50
 * handmvnet_amd/model.py mirrors that protocol and binds the entry points below through
 * ctypes (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions: plain C types only; integer status codes (0 = HMV_OK); no exceptions cross
 * the ABI; the caller owns every input/output buffer, the engine owns weights + workspace;
 * hmv_forward is asynchronous on the stream it is given (caller synchronises); a handle
 * is bound to one device and is not re-entrant; different handles are independent.
 *
 * Threading / stream contract.  One handle owns ONE workspace arena whose offsets every forward reuses (cached
 * hipGraphs bake them in), plus one set of stage-capture and profiling buffers.  A handle is therefore
 *   - not thread-safe: calls on one handle must be serialised by the caller;
 *   - single-stream at a time: a forward may be enqueued behind another forward of the SAME handle only on the same
 *     stream; to move a handle to another stream, synchronise (or event-order) the first stream before the next
 *     hmv_forward.  Two forwards of one handle in flight on two streams race on the workspace.
 * Concurrency comes from several handles (one per stream / rank), which share nothing.  Kernel selection is per call, not
 * shared state, so the hmv_op_* entries (a kernel_sel applies to that one call) may run on any thread while other threads run
 * forwards of their handles.
 * hmv_set_tensor + hmv_finalize_weights may be repeated on a live handle: finalisation synchronises the device and drops
 * every cached graph before it frees the previous weight buffers.
 */
#ifndef HANDMV_H
#define HANDMV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hmv_engine *hmv_handle;

enum { HMV_OK = 0, HMV_ERR_ARG = 1, HMV_ERR_STATE = 2, HMV_ERR_MISSING_TENSOR = 3, HMV_ERR_SHAPE = 4, HMV_ERR_HIP = 5,
       HMV_ERR_UNSUPPORTED = 6, HMV_ERR_RANGE = 7 /* a value outside the fp16 range of its mode: see "Range contract" below */ };

/* model_params["backbone"] = "resnet": backbone_type "18" | "34" | "50_paper"   (handmvnet.py:59-68)
 * model_params["backbone"] = "hrnet":  backbone_type "w40" | "w64"            (handmvnet.py:41-57, hrnet.py:430-447) */
enum { HMV_RESNET18 = 0, HMV_RESNET34 = 1, HMV_RESNET50_PAPER = 2, HMV_HRNET_W40 = 3, HMV_HRNET_W64 = 4 };
/* model_params["pos_enc"] subset of {pos2d, crop, sin}       (handmvnet.py:89-95) */
enum { HMV_POS2D = 1, HMV_POS_CROP = 2, HMV_POS_SIN = 4 };
/* model_params["use_gcn"]: JointsDecoderNN | JointsDecoderGCN (handmvnet.py:152-155) */
enum { HMV_DECODER_NN = 0, HMV_DECODER_GCN = 1 };
/* HMV_F16 = BASELINE configs[4]: conv stack in fp16 storage + fp16 MFMA with fp32 accumulation; heat-map
 * logits, soft-argmax, tokens, fusion transformer and decoder stay fp32.  I/O buffers are fp32 either way. */
/* HMV_F32X3: fp32-equivalent arithmetic on the fp16 matrix cores (every backbone).  Every fp32 value of the
 * conv stack travels as a (hi, lo) fp16 pair (hi = fp16(v), lo = fp16(v - hi); hi + lo == v to 2^-22) and every product is
 * evaluated as hi*hi + lo*hi + hi*lo with fp32 accumulation -- three 2.5 PFLOP/s fp16 MFMAs instead of one 157 TFLOP/s fp32
 * MFMA.  Same bytes in HBM as fp32.  Heat-map logits, soft-argmax, tokens, fusion and decoder are plain fp32 as always. */
enum { HMV_F32 = 0, HMV_F16 = 1, HMV_F32X3 = 2 };
/* Range contract of the three modes.
 *   HMV_F32    no range limit beyond fp32's own.
 *   HMV_F32X3  fp32-equivalent for values v with 2^-3 <= |v| < 65504 (2^-22 relative per operand).  Below 2^-3 lo = fp16(v - hi) is an fp16
 *              subnormal: a pair then carries an ABSOLUTE error of at most 2^-25 (half of fp16's subnormal step 2^-24), so a dot
 *              product over weights w has an extra error of at most ~2^-25 * sum|w| (measured on MI355X: the MFMA keeps fp16 subnormals; the
 *              sweep of tests/test_gpu_range.py holds every result to that floor down to 2^-14).  Weights are shifted out of that region at packing
 *              (a power of two per layer, undone in the fp32 epilogue), activations are not.  Above 65504 a pair cannot hold the value:
 *              every pair conversion clamps to +-65504 and reports it (sites whose values are pairs already -- max-pooling, the rows of the
 *              pair attention -- or are normalised frame pixels are not re-checked) -- a forward sets the handle's range word (hmv_range_status), an
 *              hmv_op_* entry returns HMV_ERR_RANGE with hmv_last_error(NULL) naming it.  Pairs are also what the q / k / v projections and
 *              the attention rows of the fusion transformer use in HMV_F16, so the same report covers that mode's tokens.
 *   HMV_F16    the conv stack behaves like model.half(): values cast round-to-nearest, |v| >= 65520 becomes +-inf (and propagates), no
 *              report.  hmv_finalize_weights returns HMV_ERR_RANGE, naming the state_dict key, for a folded weight with |w| >= 65520. */
/* model_params["fusion"] (handmvnet.py:137-149): "cross_attn" = CrossAttentionFusion (fusion.py:7-30, every release config);
 * "cross_attn_learnable_query" = CrossAttentionFusionLearnableQuery (fusion.py:33-49; layers.py:240-301): five blocks of
 * heads 8 x 256, a learnable 21-token probe as the query of the middle block, a positional embedding inside every block,
 * no LayerNorm around the attention.  fusion_layers is ignored for it (always 5), and so is HMV_POS_SIN. */
enum { HMV_FUSION_CROSS_ATTN = 0, HMV_FUSION_LEARNABLE_QUERY = 1 };

typedef struct hmv_config {
    int32_t struct_size;   /* sizeof(hmv_config), ABI guard */
    int32_t backbone;      /* HMV_RESNET* | HMV_HRNET_* */
    int32_t n_levels;      /* len(model_params["backbone_channels"]) */
    int32_t channels[4];   /* model_params["backbone_channels"] (ResNet: last level first; HRNet: highest resolution first) */
    int32_t num_views;     /* model_params["num_views"] */
    int32_t height, width; /* frame size the plan is built for (x.shape[-2:]); ResNet backbones: any size >= 32 (the heat map is
                            * ceil-chained like the reference's convs: resnet.py:216-254); HRNet: multiples of 32 (its fuse layers add
                            * 2^k-upsampled maps, hrnet.py:194-212, which only line up at those sizes -- the reference raises otherwise) */
    int32_t image_size;    /* data_params["image_size"]   -- config constant, handmvnet.py:252 */
    int32_t heatmap_size;  /* data_params["heatmap_size"] -- config constant, handmvnet.py:252 */
    int32_t pos_enc;       /* bitmask of HMV_POS* */
    int32_t fusion_layers; /* model_params["fusion_layers"], odd */
    int32_t decoder;       /* HMV_DECODER_* */
    int32_t dtype;         /* HMV_F32 | HMV_F16 | HMV_F32X3 */
    int32_t device;        /* HIP device ordinal */
    int32_t fusion;        /* HMV_FUSION_* */
} hmv_config;

/* Replaces HandMvNet.__init__ (handmvnet.py:28-125): validates the configuration and
 * builds the layer plan; no weights yet. */
int hmv_create(const hmv_config *cfg, hmv_handle *out);

/* Replaces one entry of load_state_dict (eval.py:46,50): `key` is the reference's
 * state_dict key, `host` fp32 data in the reference's layout (OIHW convs, [out,in]
 * linears, ...), copied.  Unknown keys (layer4.*, fc.*) are accepted and ignored. */
int hmv_set_tensor(hmv_handle h, const char *key, const float *host, const int64_t *shape, int32_t ndim);

/* After the last hmv_set_tensor: checks every key the forward reads is present with the
 * right shape (HMV_ERR_MISSING_TENSOR / HMV_ERR_SHAPE name the key in hmv_last_error; HMV_F16: HMV_ERR_RANGE names the key of a
 * folded weight that fp16 cannot hold),
 * folds BatchNorm into conv scale/bias, repacks to the MFMA-friendly K-major layout and
 * uploads.  Replaces .to(device).eval().freeze() (eval_fps.py:63-65). */
int hmv_finalize_weights(hmv_handle h);

/* Bytes of device workspace a forward of `batch` multi-view samples needs. */
size_t hmv_workspace_bytes(hmv_handle h, int32_t batch);

/* (Re)allocates the workspace for up to `batch` samples.  hmv_forward calls it on demand;
 * call it up front to keep allocation out of a timed or graph-captured region. */
int hmv_reserve(hmv_handle h, int32_t batch);

/* Fused tail kernels (fusion_kernels.hip: FeedForward + LayerNorms behind the to_out GEMM as one launch, the ChebConv decoder
 * as two) on (default) or off (the launch-per-op path; also HMV_NO_FFFUSE=1 / HMV_NO_CHEBFUSE=1 at hmv_create time).  A/B runs
 * and the equivalence test; the workspace is re-planned on the next forward. */
int hmv_set_tail_fusion(hmv_handle h, int32_t enable);

/* Cross-layer launches of the fp16 backbone at large batches: conv_stream.hip's chain (a Bottleneck's conv3 + residual and the NEXT
 * Bottleneck's conv1 + BN + ReLU, /root/reference/src/models/backbones/resnet.py:124-144, as ONE launch that computes the second conv
 * from the first one's output tile while it is still on the CU; layer1) and conv_hs.hip's pooled stem (conv1 + BN + ReLU + MaxPool2d,
 * resnet.py:218-221, as one launch), on (default) or off (one launch per op; also HMV_NO_CHAIN=1 / HMV_NO_STEMPOOL=1 in the environment).
 * Both give the same bits; A/B runs and the identity test; the workspace is re-planned on the next forward. */
int hmv_set_chain_fusion(hmv_handle h, int32_t enable);

/* HRNet fuse layers (/root/reference/src/models/backbones/hrnet.py:194-212, y_i = relu(sum_j f_ij(x_j))): the up-sampling terms of an
 * output branch (1x1 conv + BN + nearest up-sampling, j > i: always the last terms of the sum) as ONE launch where there are two or
 * more of them (hr_fuse.hip: the branch's map is read once and written once), on (default) or off (one conv launch per term, each
 * adding the running sum).  fp32 mode: equal up to the summation order inside a dot product; fp16 mode: the fused launch rounds the sum
 * to fp16 once instead of after every term.  The split-precision mode always runs one launch per term.
 * Bit 1 of `enable` (round 4; fp16-kernel modes only -- measured hr40 fp16 -1.2 %, f32x3 -0.9 %, fp32 +0.3 %): a four-branch module's lowest-resolution branch (its eight 3x3 convs) is enqueued on a second stream of the
 * handle beside the branch above it -- both are a few hundred latency-bound tiles per conv and share the CUs; forked from and joined
 * into the caller's stream by events (also under hipGraph capture), same kernels and bits.  enable: 0 neither, 1 fused fuse layers
 * only, 2 branch overlap only, 3 both (default).  A/B runs and the equivalence test; the workspace is re-planned on the next forward. */
int hmv_set_hr_fusion(hmv_handle h, int32_t enable);

/* Test hook: fills the reserved workspace with the byte `value` (0xFF: NaNs) on `stream`.  No stage may read workspace bytes that
 * an earlier stage of the SAME forward has not written, so a forward after poisoning returns the bits of one before it. */
int hmv_poison_workspace(hmv_handle h, int32_t value, void *stream);

/* Replaces HandMvNet.forward (handmvnet.py:158-266).  All pointers are DEVICE pointers.
 *   x               [B][V][3][H][W] fp32 (the reference's NCHW frames)
 *   bbox            [B][V][4]  (x1,y1,x2,y2), may be NULL unless HMV_POS_CROP
 *   intrinsic       [B][V][4]  (fx,fy,cx,cy), may be NULL unless HMV_POS_CROP
 *   joints_crop_img [B][V][21][2]  out
 *   joints_cam      [B][21][3]     out
 *   heatmap         [B][V][21][H/8][W/8] out, may be NULL (skips the NCHW copy)
 *   stream          hipStream_t (NULL = default stream) */
int hmv_forward(hmv_handle h, int32_t batch, const float *x, const float *bbox, const float *intrinsic,
                float *joints_crop_img, float *joints_cam, float *heatmap, void *stream);

/* hmv_forward for a batch whose samples have DIFFERENT CAMERAS: sample b brings view_counts[b] of the cfg.num_views views (a camera
 * dropped out, the hand left a view, or an accuracy-against-view-count table is being produced).  Its result is what the model built with
 * num_views = view_counts[b] computes from those views, fed in camera order, from the same weights: the backbone runs on the present
 * frames only, and the fusion attends over each sample's own 21 * view_counts[b] tokens, positions counted over its present views.
 *   view_counts     HOST, `batch` entries, each in [1, cfg.num_views]; read before the call returns
 *   x               [sum view_counts][3][H][W] fp32, packed sample-major, a sample's present views in camera order
 *   bbox, intrinsic [sum view_counts][4] each, packed the same way; may be NULL unless HMV_POS_CROP
 *   joints_crop_img [sum view_counts][21][2]  out
 *   joints_cam      [batch][21][3]            out
 *   heatmap         [sum view_counts][21][H/8][W/8] out, may be NULL
 * Asynchronous on `stream` like the uniform entry and without a device synchronisation: the per-sample row table is derived on the
 * host and uploaded on `stream`.  One forward is in flight per handle, as ever.  A workspace reserved for `batch` samples serves a
 * ragged call of up to `batch` samples.  Always runs eagerly (never replayed from the graph cache); records no stages -- reading a
 * stage afterwards returns HMV_ERR_STATE; the range report covers it like any forward.
 * HMV_ERR_ARG, before anything is launched, for: batch <= 0, a NULL table, a count of 0 or above cfg.num_views. */
int hmv_forward_views(hmv_handle h, int32_t batch, const int32_t *view_counts, const float *x, const float *bbox, const float *intrinsic,
                      float *joints_crop_img, float *joints_cam, float *heatmap, void *stream);

/* A camera-subset sweep (the camera ablation: "which k of the V cameras"): hmv_forward_views for n_subsets camera subsets of the SAME
 * full batch at the cost of ONE backbone pass.  Everything up to the per-frame token rows does not depend on which other views are
 * present, so it runs once on all batch * V frames; the positional encoding (by a frame's rank among the present views), the fusion
 * blocks and the decoder run once per subset.  joints_cam[s] holds the bits hmv_forward_views writes for this batch when every sample
 * brings the cameras of subset s.
 *   subset_mask     HOST uint8 [n_subsets][cfg.num_views], non-zero = the camera is present; one table for the whole batch; read
 *                   before the call returns.  Duplicate subsets are allowed
 *   x, bbox, intrinsic, joints_crop_img, heatmap: the FULL batch, exactly as for hmv_forward; both outputs are written once
 *   joints_cam      [n_subsets][batch][21][3]  out
 * The fusion runs in passes of at most max(batch, reserved batch) virtual samples (a virtual sample = one sample under one subset), so
 * that every buffer of a pass stays within the reservation; the retained token rows and a pass's packed rows come on top, and the
 * workspace grows before the first launch where that takes it past the reservation.  A subset's bits do not depend on the passes.
 * Asynchronous on `stream` and without a device synchronisation, like hmv_forward_views (one table upload).  Always eager, records no
 * stages (reading one afterwards returns HMV_ERR_STATE); the range report covers it.  With profiling on, the record list also holds one
 * bracketing record "subsets_frames" around the per-frame stage and one "subsets_tail" around every pass.
 * HMV_ERR_ARG, before anything is launched, for: batch <= 0, n_subsets < 1, a NULL table, a subset without a camera. */
int hmv_forward_subsets(hmv_handle h, int32_t batch, int32_t n_subsets, const uint8_t *subset_mask, const float *x, const float *bbox,
                        const float *intrinsic, float *joints_crop_img, float *joints_cam, float *heatmap, void *stream);

/* A reference-view sweep ("what is the pose in camera c's frame", "which camera should be the reference view"): hmv_forward_subsets
 * with the cameras of every row fed in the ORDER the row names them.  The first camera of an order is the reference view: the cross
 * block takes its queries from it, joints_cam comes out root-relative in its frame, and the sinusoidal positions count the others in
 * feed order.  joints_cam[s] holds the bits hmv_forward_views writes for this batch with its views permuted by order s: x, bbox and
 * intrinsic rows [order s] in the first k view slots and k present views per sample.  A sorted order is a subset (hmv_forward_subsets'
 * bits); the identity order over all cameras has hmv_forward's.
 *   orders          HOST int32 [n_orders][cfg.num_views]: each row lists k distinct cameras, 1 <= k <= num_views, from the left and is
 *                   padded with -1; one table for the whole batch; read before the call returns.  Duplicate orders are allowed
 *   x, bbox, intrinsic, joints_crop_img, heatmap: the FULL batch in camera order, exactly as for hmv_forward; both outputs are written once
 *   joints_cam      [n_orders][batch][21][3]  out
 * Passes, workspace, stream behaviour, eager execution, stages, the range report and the two bracketing profile records
 * ("subsets_frames", "subsets_tail") are hmv_forward_subsets': both entries share one host planner and one runner, and a sweep captures
 * no attention maps.  For the learnable-query fusion the sweep is defined by the same rule; which frame that model's output is in is a
 * property of its training, not of the engine.
 * HMV_ERR_ARG, before anything is launched, for: batch <= 0, n_orders < 1, a NULL table, an order without a camera, a camera outside
 * [0, num_views), a camera named twice in one order, a camera behind a -1. */
int hmv_forward_orders(hmv_handle h, int32_t batch, int32_t n_orders, const int32_t *orders, const float *x, const float *bbox,
                       const float *intrinsic, float *joints_crop_img, float *joints_cam, float *heatmap, void *stream);

/* Human-readable description of the last failure on this handle, or with h == NULL of the calling thread's last failed call
 * without a handle (hmv_create, the hmv_op_* entries ...): per thread, like errno. */
const char *hmv_last_error(hmv_handle h);

void hmv_destroy(hmv_handle h);

/* ---- introspection used by tests and bench.py (not part of the reference's surface) ---- */

/* Copies an intermediate of the LAST forward to a device buffer, converted to the
 * reference's layout.  stage: "feat0" [N][C][h][w], "coords_hm" [N][21][2],
 * "tokens" [B][V*21][d] (before the sinusoidal PE is added), "fused" [B][21][d].
 * Stage capture must have been enabled before that forward. */
int hmv_set_capture(hmv_handle h, int32_t enable);
int hmv_read_stage(hmv_handle h, const char *stage, float *dst_device, size_t capacity_floats, void *stream);

/* Attention maps of the fusion blocks: what the reference returns from MultiHeadAttention.forward(x, return_attention=True) and
 * MultiHeadAttentionLearnableQuery.forward(x, return_attention=True) (layers.py:202-237, 267-301) -- attn[b][h][i][j], the softmax with which
 * query i of head h draws on key j.  The forward's attention kernels never write it; a selected block gets one more launch directly behind
 * its attention launch, which recomputes the logits from the block's own q and k rows (the forward's operand order and scale, fp32 matrix
 * cores) and writes the probabilities.  In the fp16-kernel modes (HMV_F16, HMV_F32X3) the 128-wide heads' q and k exist only as fp16 (hi, lo)
 * pairs: the map is then fp32 arithmetic on float(hi) + float(lo) of those pairs -- the forward's own operands, not the registers of its
 * fp16-matrix-core attention.
 *   block_mask   bit l selects fusion block l (cross_attn: fusion_layers blocks, the cross block is (fusion_layers - 1) / 2; learnable
 *                query: 5 blocks, the probe block is 2).  0, the default, turns capture off: nothing a forward enqueues changes.  A bit at or
 *                above the block count is HMV_ERR_ARG.  A non-zero mask keeps forwards on the eager path (as stage capture does); the buffers are
 *                the handle's own, outside the workspace, and grow with hmv_reserve / the next forward.
 *   forwards     hmv_forward, hmv_forward_frames, hmv_forward_views, hmv_forward_frames_views (and their _track forms) honour the mask;
 *                hmv_forward_subsets ignores it and leaves no map.
 *   shape        of the last forward's map: probs [B][8][Tq][Tk] dense fp32; after a ragged forward Tq / Tk / views are the batch's maxima,
 *                a shorter sample's rows and columns beyond its own are zeros, and a sample with one view has no keys in cross_attn's cross
 *                block (its rows are zeros).  views: the view columns of the share, 0 for a block behind the cross block (its 21 fused keys
 *                are no views).
 *   view share   share[b][h][i][r] = the sum, in key order in fp32, of p over the 21 keys of the view of RANK r among the sample's present
 *                views; [B][8][Tq][views].  In cross_attn's cross block the keys start at the second view -- the view of rank 0 supplies the
 *                queries -- so column 0 is exactly 0 there.
 * hmv_read_attention copies device-to-device on `stream`; either destination may be NULL.  HMV_ERR_STATE: the block was not selected before
 * the last forward, or the last call was a sweep.  HMV_ERR_ARG: a capacity (in floats) smaller than the data -- nothing is truncated --, or
 * view_share for a block without one.  A single-view model's cross block has Tk = 0: the call succeeds, copies no probabilities and returns
 * a share of zeros. */
int hmv_set_attention_capture(hmv_handle h, uint32_t block_mask);
int hmv_attention_shape(hmv_handle h, int32_t block, int32_t *B, int32_t *Tq, int32_t *Tk, int32_t *views);
int hmv_read_attention(hmv_handle h, int32_t block, float *probs, size_t probs_capacity, float *view_share, size_t share_capacity,
                       void *stream);

/* Per-launch timing with hipEvents on the forward's stream (0 = off, 1 = on).  When on,
 * hmv_forward records an event pair around every kernel launch of the conv/GEMM kernel
 * family; records accumulate over successive forwards (calling hmv_set_profiling again
 * clears them; enable = 0 pauses and keeps the records, enable = 2 resumes without clearing);
 * hmv_profile_* read them back after the caller has synchronised the stream. */
int hmv_set_profiling(hmv_handle h, int32_t enable);
int hmv_profile_count(hmv_handle h);
/* name: kernel family = one device symbol ("conv_igemm_f32<256x256,1x1>" ...); label: layer ("layer3.2.conv2"; "a+b": one launch
 * for both); ms: duration; flops: 2*M*N*K of that launch over the real (un-padded) channels -- M the rows the launch computes, so a
 * SampleNet conv counts the 4 gathered pixels of each joint, not the whole map, and an up-sampling fuse term that runs alone counts
 * the up-sampled pixels (the fused form, hr_fuse.hip, multiplies at the sources' resolution and counts that). */
int hmv_profile_get(hmv_handle h, int32_t index, const char **name, const char **label, float *ms, double *flops);
/* algorithmic HBM bytes of that launch: input pixels, weights, residual and output rows each moved once in the storage type of
 * the arithmetic mode (what bench.py prices the launch's HBM roofline with).  A strided 1x1 reads only the pixels it keeps; a pooled
 * launch never moves the conv map; a dual launch reads each source at the pixels it uses; a (hi, lo) pair is 4 bytes; the fused
 * up-sampling launch of an HRNet fuse layer keeps fp32 weights in every mode (4 bytes each).  tests/test_gpu_launch_ledger.py
 * recomputes flops and bytes of every launch of the benchmarked forwards from these sentences. */
int hmv_profile_get_bytes(hmv_handle h, int32_t index, double *bytes);
/* Device operations (kernel launches, memsets, device-to-device copies) that the last eagerly run forward of this handle
 * enqueued: the "launches per forward" figure of bench.py (a hipGraph replay enqueues ONE graph of as many nodes). */
int hmv_launch_count(hmv_handle h);

/* Range report of the (hi, lo) pair modes (HMV_F32X3; the fusion transformer of HMV_F16): synchronises `stream`, sets *saturated to 1 if any
 * forward of this handle since the last call clamped a value to the pair range (|v| > 65504, see "Range contract"), else 0, and clears it.
 * Sticky: one call after an evaluation loop covers every forward in it.  The forward itself adds nothing for it (no launch, memset or
 * synchronisation; the word lives outside the workspace, so hmv_poison_workspace and cached graphs leave it alone). */
int hmv_range_status(hmv_handle h, int32_t *saturated, void *stream);

/* Op-level entries.  For every device pointer of these entries -- and of every other entry of this header -- a caller may rely on this:
 * bytes outside an operand never influence a result, bytes outside an output are never written, and inputs are never modified. */

/* One NHWC convolution through the engine's conv kernel (op-level parity tests).
 * in [N][H][W][Cin] device; weight OIHW host (Cin must be a multiple of 4);
 * bias host[Cout] or NULL; residual device [N][Ho][Wo][Cout] or NULL; out device NHWC. */
int hmv_op_conv2d(int32_t device, const float *in, int32_t N, int32_t H, int32_t W, int32_t Cin,
                  const float *weight_oihw_host, const float *bias_host, int32_t Cout, int32_t R, int32_t S,
                  int32_t stride, int32_t pad, const float *residual, int32_t relu, float *out, void *stream);

/* The same op in any arithmetic mode (dtype = HMV_F32 | HMV_F16 | HMV_F32X3): the fp32 input / residual are converted to the
 * mode's storage format on the device, the layer is packed exactly as hmv_finalize_weights packs it (no BatchNorm), the
 * output is fp32.  Cin must be a multiple of 8 for the fp16-based modes.  HMV_F32X3: HMV_ERR_RANGE when a value was clamped to the
 * pair range (also hmv_op_conv2d_x3, hmv_op_attention_x3); HMV_F16 (also hmv_op_conv2d_f16): out-of-range values become +-inf. */
int hmv_op_conv2d_ex(int32_t device, int32_t dtype, const float *in, int32_t N, int32_t H, int32_t W, int32_t Cin,
                     const float *weight_oihw_host, const float *bias_host, int32_t Cout, int32_t R, int32_t S, int32_t stride,
                     int32_t pad, const float *residual, int32_t relu, float *out, void *stream);

/* One fp32 3x3 stride-1 pad-1 conv C -> C (+ bias, optional residual / ReLU) in the engine's ROW-DECOMPOSED packing -- what HRNet-w40's
 * 40- and 80-channel branch convs run (hrnet.py:96-221).  C % 4 == 0, C % 32 != 0, 3 C <= 256, 128 % W == 0.  kernel_sel: 0 = the
 * launcher's choice, 1 = conv_igemm's row-decomposed tiles, 2 = the persistent weight-stationary kernel (conv_rds.hip; C = 40 / 80,
 * 64 % W == 0) whatever the size.  *kernel_name (optional) receives the family that ran. */
int hmv_op_conv2d_rd(int32_t device, const float *in, int32_t N, int32_t H, int32_t W, int32_t C, const float *weight_oihw_host,
                     const float *bias_host, const float *residual, int32_t relu, float *out, int32_t kernel_sel,
                     const char **kernel_name, void *stream);

/* hmv_op_conv2d_ex (fp32 output rows in every mode, the launcher's own kernel choice) in the launch geometries and packings of the
 * engine that the other entries cannot express, with the kernel family reported (op-level tests at the benchmarked shapes):
 *   Ho, Wo > 0: only the top-left Ho x Wo of the conv's output map is computed (<= the conv's own size; residual and `out` are
 *               [N][Ho][Wo][Cout]) -- how the ResNet stem runs: a 4x4 pad-2 conv over 2x2 space-to-depth frames cut to H x W;
 *               0 = the conv's own size.
 *   packing 1:  the ROW-DECOMPOSED packing of hmv_op_conv2d_rd for Cin != Cout as well (HRNet-w40's transition 256 -> 40): HMV_F32, 3x3
 *               stride 1 pad 1, Cout % 4 == 0, 3 Cout <= 256, 128 % W == 0, Ho = Wo = 0; the bias is then applied as a BatchNorm shift.
 *               0 = the plain packing.
 * HMV_F16: what a layer of the fp16 path that writes fp32 rows runs (heat-map logits, SampleNet rows). */
int hmv_op_conv2d_as(int32_t device, int32_t dtype, const float *in, int32_t N, int32_t H, int32_t W, int32_t Cin,
                     const float *weight_oihw_host, const float *bias_host, int32_t Cout, int32_t R, int32_t S, int32_t stride,
                     int32_t pad, const float *residual, int32_t relu, float *out, int32_t Ho, int32_t Wo, int32_t packing,
                     const char **kernel_name, void *stream);

/* hmv_op_conv2d with a kernel selector (op-level parity tests): 0 = the launcher's choice, 1 = conv_igemm only, 2 = the persistent
 * weight-stationary kernel (conv_stream.hip, fp32 variant: residual-bearing 1x1 convs with K = 64 / 128 / 256, Cout % 256 == 0)
 * wherever the shape has one, whatever its size.  *kernel_name (optional) receives the family that ran. */
int hmv_op_conv2d_sel(int32_t device, const float *in, int32_t N, int32_t H, int32_t W, int32_t Cin,
                      const float *weight_oihw_host, const float *bias_host, int32_t Cout, int32_t R, int32_t S, int32_t stride,
                      int32_t pad, const float *residual, int32_t relu, float *out, int32_t kernel_sel, const char **kernel_name,
                      void *stream);

/* The fp16-storage op with fp16 OUTPUT rows (what a backbone layer of the fp16 path writes): out_f16 device [N][Ho][Wo][Cout]
 * halfs.  kernel_sel: 0 = the launcher's choice, 1 = conv_igemm only, 2 = the round-3 kernels (conv_stream.hip: persistent
 * weight-stationary residual 1x1; conv_gemm8.hip: phase-interleaved 256 x 256 1x1; conv_hs.hip: halo-streaming few-channel 3x3)
 * wherever the shape has one, whatever its size; 3 = the tall-tile 3x3 kernel (conv_ht.hip: 3x3 stride 1 pad 1 without residual,
 * Cin % 32 == 0 >= 64, Cout % 128 == 0, H % 16 == 0, W % 32 == 0, else HMV_ERR_ARG) with the weights packed in ITS reduction order,
 * as hmv_finalize_weights packs the layers the engine gives to it, on the 16x16x32 fp16 MFMA (the engine's shape since round 4);
 * 4 = the same packing on the small-launch tiles (conv_m16.hip: what such a layer runs on when the batch is too small for
 * 512-pixel tiles: same bits as 3); 5 / 6 = as 3 / 4 on the 32x32x16 fp16 MFMA (conv_ht's other instantiation / conv_igemm's
 * 32-channel-chunk tiles: the partner of the MFMA-shape A/B of round 4, not used by the engine; 5 and 6 agree bit for bit with
 * each other, and with 3 / 4 to the last fp16 bit of a few outputs); 7 = as 3 on conv_ht's PERSISTENT form (one workgroup per CU walks
 * its tiles with the next tile's operands in flight; what a launch of two or more tiles per CU runs on; 3 is one workgroup per tile
 * whatever the size; same bits; channel-tile counts other than 1, 2, 4 have no persistent form and run as 3); 8 = as 2 with conv_gemm8's
 * PERSISTENT form wherever it exists (2 is one workgroup per tile whatever the size; same bits).  *kernel_name (optional) receives the family that ran.
 * Cout % 4 == 0; output rows that are no whole 16-byte vectors (Cout % 8 != 0: no backbone layer has them) run on conv_igemm's staged
 * epilogue, whatever Cin is.  The kernel_sel of the hmv_op_* entries applies to that call alone. */
int hmv_op_conv2d_f16(int32_t device, const float *in, int32_t N, int32_t H, int32_t W, int32_t Cin,
                      const float *weight_oihw_host, const float *bias_host, int32_t Cout, int32_t R, int32_t S, int32_t stride,
                      int32_t pad, const float *residual, int32_t relu, void *out_f16, int32_t kernel_sel,
                      const char **kernel_name, void *stream);

/* hmv_op_conv2d_ex(dtype = HMV_F32X3) with a kernel selector for the split-pair token GEMMs with a short reduction (the q / k / v
 * projections of the fp16-kernel modes: layers.py:213-215): 0 = the launcher's choice (gemm_x3.hip's 256 x 256 tiles from ~200 tiles
 * up, conv_igemm's fused split loop below), 1 = conv_igemm's fused split loop only, 2 = gemm_x3k16 whenever the shape allows.  The two
 * give the same bits.  fp32 output rows; *kernel_name (optional) receives the family that ran. */
int hmv_op_conv2d_x3(int32_t device, const float *in, int32_t N, int32_t H, int32_t W, int32_t Cin,
                     const float *weight_oihw_host, const float *bias_host, int32_t Cout, int32_t R, int32_t S, int32_t stride,
                     int32_t pad, const float *residual, int32_t relu, float *out, int32_t kernel_sel, const char **kernel_name,
                     void *stream);

/* One conv / GEMM launch in a LAUNCH FORM that only the engine's forward issues otherwise (op-level float64 tests: tests/test_gpu_conv_forms.py):
 * packed by the loader members the model loader calls (identity BatchNorm folds), launched through the engine's own launch path, temporaries
 * framed by guard bands.  `form` is a sum of HMV_FORM_* bits; 0 is the plain launch of hmv_op_conv2d_ex.  Every device operand is fp32 rows
 * (converted to the mode's storage format first, pad columns included); weights and biases are on the host.
 *   in        [N][H][W][ld_in]: ld_in = 0 or Cin, or more: the map then has ld_in physical channels of which Cin are real, as the loader's
 *             padded layers have (the stem's 12 of 16); the extra channels meet zero weights and must be finite.  Dual: ld_in = Cin only.
 *   residual  [N][Ho][Wo][ldr] or NULL; out [N][Ho][Wo][ldc]: fp32 rows in HMV_F32 and HMV_F32X3, fp16 rows in HMV_F16.  Columns from Cout on
 *             are never written.  Ho, Wo = 0: the conv's own map; else its top-left Ho x Wo (hmv_op_conv2d_as).
 *   route_*   per kernel family: 0 the launcher's rule, 1 never, 2 whenever the shape has an instantiation (ROUTE_FORCE);
 *             gemm8_persist: 0 the rule, 1 never, 2 wherever the persistent form exists.
 *   HMV_FORM_DUAL    1x1 only: out = act([in | in2(strided)] . [w ; w2] + bias + bias2), in2 [N][H2][W2][ld_in2] with Cin2 real channels
 *                    sampled at (ho * stride2, wo * stride2), w2 [Cout][Cin2].  HMV_F32 / HMV_F16, whole 32 / 64-channel chunks per source.
 *   HMV_FORM_CHAIN   HMV_F16: the launch also writes next_out [M][next_cout] fp16 = relu(conv1x1(fp16 out, next_w [next_cout][Cout]) +
 *                    next_bias), where the engine's rule for its own launches (under the given route) chains; with or without DUAL.
 *   HMV_FORM_POOL    HMV_F16: MaxPool2d(3, 2, 1) of the conv map in the same launch; out is the pooled map [N][pool_h][pool_w][ldc].
 *   HMV_FORM_PHASES  w is a ConvTranspose2d(4, 2, 1) weight [Cin][Cout][4][4] (R = S = 4, stride 2, pad 1 describe it); out
 *                    [N][2 H][2 W][ldc].  merged 0: four phase launches; 1: the one launch over the four weight blocks (not with pairs).
 *   HMV_FORM_SPLITK  HMV_F32 1x1: `slices` partial products over the reduction columns [i Kpad / slices, (i + 1) Kpad / slices), without
 *                    bias, into out [slices][M][ldc]; slices is 1 or what the engine's rule gives the layer.
 *   HMV_FORM_PAIR_OUT  HMV_F32X3: out receives [hi ldc | lo ldc] fp16 rows; HMV_ERR_RANGE when the range word was raised.
 * kernel_name receives the family of the (last) launch.  HMV_ERR_ARG, naming the entry, before any launch for a NULL args, another
 * struct_size, a NULL or non-positive operand, a form or stride the engine never issues; a launch the launcher refuses is HMV_ERR_HIP. */
enum { HMV_FORM_DUAL = 1, HMV_FORM_CHAIN = 2, HMV_FORM_POOL = 4, HMV_FORM_PHASES = 8, HMV_FORM_SPLITK = 16, HMV_FORM_PAIR_OUT = 32 };
typedef struct hmv_conv_form_args {
    int32_t struct_size;   /* sizeof(hmv_conv_form_args) */
    int32_t dtype, form;
    int32_t N, H, W, Cin, Cout, R, S, stride, pad, relu;
    int32_t Ho, Wo;
    int32_t ld_in, ldc, ldr, ld_in2;
    int32_t route_stream, route_gemm8, route_hs, route_x3k16, gemm8_persist;
    int32_t Cin2, H2, W2, stride2;   /* dual */
    int32_t next_cout;               /* chain */
    int32_t pool_h, pool_w;          /* pool */
    int32_t merged;                  /* phases */
    int32_t slices;                  /* split-K */
    int32_t reserved;
    const float *in, *residual, *in2;           /* device */
    const float *w, *bias, *w2, *bias2;         /* host */
    const float *next_w, *next_bias;            /* host */
    void *out, *next_out;                       /* device */
    const char *kernel_name;                    /* out */
} hmv_conv_form_args;

int hmv_op_conv2d_form(int32_t device, hmv_conv_form_args *args, void *stream);

/* The up-sampling terms of an HRNet fuse layer (hrnet.py:194-212) through hr_fuse.hip alone (op-level parity tests; the fp16 instantiation
 * needs row strides of whole 16-byte units: ldc % 8 == 0, source ld % 8 == 0):
 *   out = act(base + sum_s Upsample_{2^shift_s, nearest}(W_s x_s + b_s)),   terms added in the order given (1 <= nsrc <= 3, 1 <= shift <= 3).
 * base [N][H][W][C] and src[s] [N][H >> shift_s][W >> shift_s][src_c[s]]: device fp32 NHWC; w_host[s] [C][src_c[s]] and bias_host[s] [C] on
 * the host.  f16 != 0: the fp16 instantiation on fp16 copies of base / src, `out` receives fp16 rows; else fp32 rows.  HMV_ERR_ARG for
 * shapes without a fused form (C % 4 -- fp16: 8 --, src_c % 16, map sizes that are not exact multiples of 2^shift). */
int hmv_op_hr_fuse_up(int32_t device, int32_t f16, const float *base, int32_t N, int32_t H, int32_t W, int32_t C, int32_t nsrc,
                      const float *const *src, const int32_t *src_c, const int32_t *shift, const float *const *weight_host,
                      const float *const *bias_host, int32_t relu, void *out, void *stream);

/* One multi-head attention of the fusion transformer (layers.py:216-221; 8 heads x 128) through the engine's kernel
 * (op-level parity tests).  qkv device [B][T][3 * 1024] = [q | k | v] per token; queries are tokens [0, Tq), keys / values
 * tokens [koff, koff + Tk); out device [B][Tq][1024]. */
int hmv_op_attention(int32_t device, const float *qkv, int32_t B, int32_t T, int32_t Tq, int32_t koff, int32_t Tk, float *out,
                     void *stream);
/* The same attention as the fp16-kernel modes (HMV_F16, HMV_F32X3) run it: q, k, v, P as fp16 (hi, lo) pairs on the fp16 matrix cores,
 * three products per step, fp32 accumulation and softmax -- fp32-equivalent: q, k, v to 2^-22 relative (the pair range above), P, which
 * reaches down to 0, as the pair of 2^14 P with an ABSOLUTE quantum of 2^-39 (fp16's subnormal spacing; unscaled it was 2^-25, and a key
 * with P below that was dropped whatever its value row held).  Same arguments; the fp32 rows are split into pairs first (in those modes the
 * projection GEMMs write pairs themselves); synchronises the stream. */
int hmv_op_attention_x3(int32_t device, const float *qkv, int32_t B, int32_t T, int32_t Tq, int32_t koff, int32_t Tk, float *out,
                        void *stream);
/* The same two kernels with their `pairs` epilogue (what a forward of the fp16-kernel modes with the fused tail launches; op-level tests):
 * x3 = 0 the fp32 kernel of hmv_op_attention, x3 = 1 the pair kernel of hmv_op_attention_x3 (the fp32 rows are split first).  out_pairs:
 * device [B][Tq][hi 1024 | lo 1024] halfs, hi = fp16(clamp(v, +-65504)), lo = fp16(clamped - hi) of the fp32 row the same kernel stores
 * without the epilogue.  sat (or NULL): device range word, set to 1 by the fp32 kernel where a row value was clamped and left alone
 * otherwise; the pair kernel never writes it (its rows are convex combinations of values that are pairs already) -- there the entry's own
 * split of the inputs reports, as HMV_ERR_RANGE.  Synchronises the stream. */
int hmv_op_attention_pairs(int32_t device, int32_t x3, const float *qkv, int32_t B, int32_t T, int32_t Tq, int32_t koff, int32_t Tk,
                           void *out_pairs, int32_t *sat, void *stream);

/* The attention of the learnable-query fusion (MultiHeadAttentionLearnableQuery, layers.py:284-291; 8 heads x 256) through the
 * engine's kernel: q rows at q + (b * q_bstride + i) * q_ld (q_bstride = 0: the same probe queries for every sample), k / v rows
 * at k + (b * T + j) * kv_ld, j < T; softmax(q k^T / 16) v per (sample, head); out device [B][Tq][2048].  QK^T and PV run
 * on the fp32 matrix cores (the kernel template of the 128-wide heads at D = 256). */
int hmv_op_attention_lq(int32_t device, const float *q, int32_t q_ld, int32_t q_bstride, const float *k, const float *v, int32_t kv_ld,
                        int32_t B, int32_t T, int32_t Tq, float *out, void *stream);

/* The ragged forms of the three attention kernels on their own (what the ragged forward launches; op-level tests).  seg: HOST table of
 * B + 1 first rows -- sample b owns rows seg[b] .. seg[b + 1] of the packed row matrix; seg[0] = 0.
 *   kind 0  128-wide heads, fp32 matrix cores;  kind 1  the same over fp16 (hi, lo) pairs (the rows are split first);
 *           qkv device [rows][3 * 1024] = [q | k | v] per row.  cross = 0: every row queries its sample's rows, out [rows][1024];
 *           cross = 1: a sample's first 21 rows query the REST of its rows, out [B * 21][1024] -- exact zeros for a sample of 21 rows
 *   kind 2  256-wide heads.  cross = 0: qkv device [rows][3 * 2048], out [rows][2048];  cross = 1: qkv holds [k | v] rows
 *           [rows][2 * 2048], the queries are the 21 rows of `probe` [21][2048] for every sample, out [B * 21][2048]
 * Synchronises the stream. */
int hmv_op_attention_views(int32_t device, int32_t kind, const float *qkv, const float *probe, int32_t B, const int32_t *seg, int32_t cross,
                           float *out, void *stream);

/* The attention-map kernels on their own (what a forward launches under hmv_set_attention_capture; op-level tests).
 *   kind 0  128-wide heads over fp32 rows;  kind 1  the same over fp16 (hi, lo) pairs (the fp32 rows are split first);  qkv device
 *           [rows][3 * 1024] = [q | k | v] per row
 *   kind 2  256-wide heads: probe == NULL: qkv device [rows][3 * 2048];  probe != NULL: qkv holds [k | v] rows [rows][2 * 2048] and the
 *           queries are the Tq rows of `probe` [Tq][2048] for every sample
 * seg == NULL, a uniform batch of B samples of T rows: the first Tq rows of a sample (or the probe's) query its rows [koff, koff + Tk);
 * probs device [B][8][Tq][Tk].  seg != NULL, a HOST table of B + 1 first rows (seg[0] = 0; T and Tk are not read): Tq = 0: every row of a
 * sample queries, Tq > 0: its first Tq rows (or the probe's) do; the keys are its rows from koff on; probs device
 * [B][8][Tq or the longest sample][the longest sample - koff], zero-filled by the call, exact zeros beyond a sample's own extent.
 * view_share (or NULL): device [B][8][that Tq][views], the share per view as hmv_read_attention describes it, key 0 belonging to the view
 * of rank koff / 21; needs koff % 21 == 0 and key ranges of whole views.
 * HMV_ERR_ARG before any launch, with hmv_last_error(NULL) naming it, for a range that would read outside the rows described (Tq > T,
 * koff + Tk > T, a sample shorter than koff or Tq), non-positive sizes and a probe with another kind.  Synchronises the stream. */
int hmv_op_attention_probs(int32_t device, int32_t kind, const float *qkv, const float *probe, int32_t B, int32_t T, int32_t Tq, int32_t koff,
                           int32_t Tk, const int32_t *seg, float *probs, float *view_share, int32_t views, void *stream);

/* ---- the non-GEMM kernels of a forward, each behind the launcher the engine calls (op-level float64 tests) ----
 * Every operand is a DEVICE pointer.  Each entry checks its arguments (HMV_ERR_ARG with hmv_last_error(NULL) naming the entry, before any
 * launch), runs one launcher on `stream` and synchronises it.  Nothing is allocated, nothing outlives the call.  `sat` (optional) is a range
 * word as "Range contract" describes it: set to 1 when a value was clamped to the pair range, left alone otherwise. */

/* Frames x [N][3][H][W] fp32 -> the stem's input rows.  kind 0, one row per pixel: mode 0 fp32 [r g b 0]; 1 fp16 [r g b 0 0 0 0 0];
 * 2 split pairs [hi: r g b 0 x5 | lo: r g b 0 x5].  kind 1, one row per 2x2 pixel block of the (H + 1) / 2 x (W + 1) / 2 space-to-depth image,
 * channel order (dy, dx, c), zeros beyond an odd H / W: mode 0 fp32 [12]; 1 fp16 [12 + 4 zeros]; 2 split pairs [hi 16 | lo 16]. */
int hmv_op_input_layout(int32_t device, int32_t kind, int32_t mode, const float *x, int32_t N, int32_t H, int32_t W, void *out, int32_t *sat,
                        void *stream);

/* MaxPool2d(3, 2, 1) over NHWC rows in the kernel's own format: mode 0 fp32 [C] (C % 4 == 0); 1 fp16 [C]; 2 split pairs [hi C | lo C]
 * (C % 8 == 0): the maximum of hi + lo, split again.  out [N][(H - 1) / 2 + 1][(W - 1) / 2 + 1] rows.  Finite inputs: the fp16 pool starts
 * from -65504, not -inf. */
int hmv_op_maxpool(int32_t device, int32_t mode, const void *in, int32_t N, int32_t H, int32_t W, int32_t C, void *out, void *stream);

/* soft_argmax_2d at temperature 1000 over channels-last logits hm [N * h * w][ld] (21 joint channels, ld >= 21): coords [N][21][2] in
 * heat-map pixels, crop_img = coords * image_size / heatmap_size, hm_nchw (or NULL) [N][21][h][w] the logits transposed. */
int hmv_op_soft_argmax(int32_t device, const float *hm, int32_t ld, int32_t N, int32_t h, int32_t w, float *coords, float *crop_img,
                       float image_size, float heatmap_size, float *hm_nchw, void *stream);

/* SampleNet's grid_sample(align_corners=True, zeros padding) as gather -> (pointwise conv) -> blend, on maps of at least 2 x 2 pixels.
 * gather: feat [N][H][W] pixel rows of C elements of elem_bytes (4: fp32 or split pairs, 2: fp16; whole 16-byte chunks) -> out
 * [(n * 21 + j) * 4 + tap] rows, taps nw, ne, sw, se of coords [N][21][2]; a tap outside the map, or any tap of a non-finite coordinate, is zeros.
 * blend: s4 [(n * 21 + j) * 4 + tap][lds4] -> tokens[n * 21 + j][col0, col0 + C) = the bilinear blend; no other column is written. */
int hmv_op_sample_gather(int32_t device, const void *feat, int32_t N, int32_t H, int32_t W, int32_t C, int32_t elem_bytes, const float *coords,
                         void *out, void *stream);
int hmv_op_sample_blend(int32_t device, const float *s4, int32_t lds4, int32_t C, int32_t N, int32_t H, int32_t W, const float *coords,
                        float *tokens, int32_t ldt, int32_t col0, void *stream);

/* The token tail, in place on tokens [N * 21][ldt] whose first fdim columns hold the features: pos2d columns (pos_mask & HMV_POS2D: coords),
 * crop FoV columns (HMV_POS_CROP: bbox, intr [N][4]), zeros in [d, ldt), d = fdim + 2 + 10 as selected; then raw_copy (or NULL) [N * 21][d] =
 * the row, + pe (or NULL) [positions][d], and pairs (or NULL) [N * 21][hi ldt | lo ldt] fp16 = the finished row split.  fpos == NULL: frame n
 * is view n % V, position (n % V) * 21 + j;  fpos device [N]: position fpos[n] + j (the ragged form, no raw_copy). */
int hmv_op_tokens_finalize(int32_t device, float *tokens, int32_t ldt, int32_t d, int32_t fdim, int32_t N, int32_t V, const int32_t *fpos,
                           const float *coords, const float *bbox, const float *intr, int32_t pos_mask, const float *pe, float *raw_copy,
                           void *pairs, int32_t *sat, void *stream);

/* y = LayerNorm(x; g1, b1) over d <= 1024 columns, eps 1e-5, zeros in [d, ldy) (ldy <= 1024); with g2, b2, y2 (all or none):
 * y2 = LayerNorm(y; g2, b2) as well. */
int hmv_op_layernorm(int32_t device, const float *x, int32_t ldx, int32_t rows, int32_t d, const float *g1, const float *b1, float *y, int32_t ldy,
                     const float *g2, const float *b2, float *y2, void *stream);

/* The epilogues of a split-K GEMM over slab [S][rows][lds]: v = slices added in index order + bias + res (or NULL; row r reads res row
 * (r / rg_out) * rg_in + r % rg_out, rg_out = 0: row r), then act (0 none, 1 ReLU, 2 GELU, 3 LeakyReLU 0.01) -> out[r][0, N);
 * or (S = 4 only) hmv_op_layernorm of v, bit for bit what the two calls in a row give. */
int hmv_op_splitk_reduce(int32_t device, const float *slab, int32_t S, int32_t rows, int32_t lds, int32_t N, const float *bias, const float *res,
                         int32_t ldr, int32_t rg_out, int32_t rg_in, int32_t act, float *out, int32_t ldc, void *stream);
int hmv_op_splitk_layernorm(int32_t device, const float *slab, int32_t S, int32_t rows, int32_t lds, int32_t d, const float *bias,
                            const float *res, int32_t ldr, int32_t rg_out, int32_t rg_in, const float *g1, const float *b1, float *y, int32_t ldy,
                            const float *g2, const float *b2, float *y2, void *stream);

/* y[r][0, d) = x[r][0, d) + pe[pos(r)][0, d), zeros in [d, ldy).  fpos == NULL: pos = r % T;  fpos device [rows / 21]:
 * pos = fpos[r / 21] + r % 21 (rows % 21 == 0). */
int hmv_op_add_pe(int32_t device, const float *x, int32_t ldx, int32_t rows, int32_t T, const int32_t *fpos, int32_t d, const float *pe, float *y,
                  int32_t ldy, void *stream);

/* ChebConv mix: out[b * 21 + i][o] = act(sum_k sum_j tk[k][i][j] * y[b * 21 + j][k * co + o] + bias[o]), k < 3, o < co; leaky: LeakyReLU 0.01.
 * tk [3][21][21]; ldy >= 3 co, ldo >= co; no column from co on is written. */
int hmv_op_cheb_mix(int32_t device, const float *y, int32_t ldy, int32_t B, int32_t co, const float *tk, const float *bias, int32_t leaky,
                    float *out, int32_t ldo, void *stream);

/* The fused tail of a fusion block, everything behind its to_out GEMM in one launch (launch_ff_block):
 *   t  = slab: slices 0 .. S - 1 added in index order + bias0 + res row (or no res)   |   x: the row as it is
 *   n1 = n1g ? LayerNorm(t; n1g, n1b) : t;   f0 = LayerNorm(n1; fg, fb);   h = GELU(f0 W1^T + b1);   f2 = h W2^T + b2 + n1
 *   out = n2g ? LayerNorm(f2; n2g, n2b) : f2, columns [d, ldo) written as zeros; out_pairs (or NULL) [rows][hi ldo | lo ldo] fp16 =
 *   the same rows split, `sat` (or NULL) raised when a value was clamped to the pair range.
 * Exactly one of slab / x.  slab [S][rows][lds], S in 1 .. 4, slice s at slab + s * slice (floats); bias0 has round4(d) floats; res row of
 * output row r is (r / rg_out) * rg_in + r % rg_out (rg_out = 0: r), stride ldr.  Rows of slab, res and x are read up to round4(d), nothing
 * beyond it, and what [d, round4(d)) holds changes no result.
 * Operand contract of the kernel: w1 is [hid][ldw1], ldw1 >= ld, finite in columns [d, ld) (they meet zeros); w2 has at least ld rows of
 * ldw2 >= hid floats, zeros in rows [d, ld); b1 has hid floats; b2 has ld floats, zeros past d; every gamma and beta has d floats; every row
 * stride (lds, ldr, ldx, ldw1, ldw2, ldo) is a multiple of 4; d <= ld = ldo <= 576, ld % 16 == 0, hid 128 or 256.  n1g / n1b and n2g / n2b
 * come in pairs or not at all.
 * tile_rows: 0 = the launcher's rule (32-row tiles once ceil(rows / 16) exceeds the device's CU count and they fit LDS, else 16);
 * 16 or 32 forces a height (32 is refused where it does not fit 160 KB of LDS: ld > 544 at hid 128, ld > 480 at hid 256).  A row's bits
 * depend on neither the height nor the row's place in the call.  tile_rows_used receives the height launched (args is not const).
 * HMV_ERR_ARG before any launch for a NULL args, another struct_size, everything above that does not hold, rows < 1, d < 1, lds / ldr /
 * ldx below d, rg_out < 0 or 0 < rg_in < rg_out, a NULL out, w1, w2, b1, b2, fg or fb. */
typedef struct hmv_ff_block_args {
    int32_t struct_size;   /* sizeof(hmv_ff_block_args) */
    int32_t rows, d, ld, hid;
    int32_t S, lds, ldr;
    int64_t slice;
    int32_t rg_out, rg_in, ldx, ldw1, ldw2, ldo;
    int32_t tile_rows;        /* in */
    int32_t tile_rows_used;   /* out */
    const float *slab, *bias0, *res, *x;
    const float *n1g, *n1b, *fg, *fb;
    const float *w1, *b1, *w2, *b2;
    const float *n2g, *n2b;
    float *out;
    void *out_pairs;
    int32_t *sat;
} hmv_ff_block_args;

int hmv_op_ff_block(int32_t device, hmv_ff_block_args *args, void *stream);

/* JointsDecoderGCN as the engine runs it, two launches (launch_cheb_fused): three ChebConv layers K -> c1 -> c2 -> c3 over x [B * 21][ldx],
 *   layer_i(v)[b * 21 + n][o] = sum_k sum_j tk[k][n][j] * (v_b W_i,k)[j][o] + bias_i[o],  LeakyReLU 0.01 after layers 1 and 2.
 * w_i: [3 * c_i][ldw_i], row k * c_i + o = column o of order k's weight; w3 has 16 rows, zeros from row 3 * c3 on.  tk [3][21][21].
 * scratch [B * 21][c1] receives layer 1's output, out[b * 21 + n][0, c3) the result (stride ldo; no other column is written).
 * Shapes (cheb_fusable): K <= 576, K % 16 == 0, c1 <= 256, c1 % 16 == 0, c2 <= 64, c2 % 16 == 0, c3 <= 5, ldx / ldw1 >= K, ldw2 >= c1,
 * ldw3 >= c2, strides multiples of 4.  A sample's bits do not depend on B.
 * HMV_ERR_ARG before any launch for a NULL args, another struct_size, a shape outside that list, a size below 1, ldo < c3, a NULL pointer. */
typedef struct hmv_cheb_fused_args {
    int32_t struct_size;   /* sizeof(hmv_cheb_fused_args) */
    int32_t B, K, ldx;
    int32_t c1, ldw1, c2, ldw2, c3, ldw3;
    int32_t ldo, reserved;
    const float *x;
    const float *w1, *bias1, *w2, *bias2, *w3, *bias3;
    const float *tk;
    float *scratch;
    float *out;
} hmv_cheb_fused_args;

int hmv_op_cheb_fused(int32_t device, const hmv_cheb_fused_args *args, void *stream);

/* Diagnostic micro-benchmark: average milliseconds of `iters` launches of one NHWC conv shape on
 * pseudo-random data.  tile: -1 = the engine's own choice, else 0..7 = 128x32, 128x64, 128x128, 256x128,
 * 128x256, 256x256, 128x128 (k-step 16), 128x256 (k-step 16) (BM x BN); a value without an instantiation returns an error.
 * HMV_BENCH_CLOCK=1 adds in-kernel clock stamps (stderr). */
int hmv_bench_conv(int32_t device, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t R, int32_t S,
                   int32_t stride, int32_t pad, int32_t with_residual, int32_t tile, int32_t iters, float *avg_ms);

/* hipGraph replay (opt-in: hmv_set_graphs(h, 1) or HMV_GRAPHS=1 in the environment; it saves host time per forward,
 * not GPU time -- measured throughput on MI355X is the same as eager launches).
 * A forward whose batch and caller buffers (x / frames, bbox, intrinsic and the three outputs) equal those of an
 * earlier call is captured into a hipGraph on its second occurrence and replayed as ONE launch afterwards
 * (up to 8 buffer sets per handle, least recently used evicted).  Results are bit-identical to the eager path;
 * stage capture and profiling force the eager path.  hmv_graph_stats reports cached graphs / replays so far. */
int hmv_set_graphs(hmv_handle h, int32_t enable);
int hmv_graph_stats(hmv_handle h, int32_t *cached, int64_t *replays);

/* hmv_forward from raw camera frames: the reference prepares every view on DataLoader workers
 * (datasets/ho3d.py:35-40, 136-149: crop_and_pad_image (datasets/utils.py:40-77) -> ToTensor -> Resize((S,S), antialias=True)
 * -> Normalize(mean, std)); here that is one kernel in front of the stem conv and the fp32 NCHW batch never exists.
 * frames: device uint8 [batch*V][frame_h][frame_w][3] (HWC, the channel order the weights were trained on);
 * crop_boxes: device int32 [batch*V][4] = x1,y1,x2,y2 of the (square or not) crop window in frame pixels -- may leave the
 * frame (zeros are read there); an EMPTY window (x2<=x1 or y2<=y1, or wider than 65536 px) yields the reference's black "no visible joint" view;
 * mean/std: host float[3] (ho3d.py:38-39 uses the ImageNet constants).  The window is resized to cfg.height x cfg.width.
 * bbox / intrinsic / outputs / stream exactly as hmv_forward (bbox is normally crop_boxes as fp32, ho3d.py:198). */
int hmv_forward_frames(hmv_handle h, int32_t batch, const uint8_t *frames, int32_t frame_h, int32_t frame_w, const int32_t *crop_boxes,
                       const float *mean, const float *std, const float *bbox, const float *intrinsic, float *joints_crop_img,
                       float *joints_cam, float *heatmap, void *stream);

/* hmv_forward_views from raw camera frames: hmv_forward_views with the frame preparation of hmv_forward_frames in front instead of an
 * fp32 batch.  The uint8 frames are neither copied nor gathered: `frames` and `crop_boxes` stay in the caller's full layout,
 *   frames      device uint8 [batch * cfg.num_views][frame_h][frame_w][3],  crop_boxes  device int32 [batch * cfg.num_views][4],
 * and packed frame n (sample-major, a sample's present views in camera order) is prepared from frames[frame_index[n]] with the
 * window crop_boxes[frame_index[n]].
 *   view_counts     HOST, `batch` entries, each in [1, cfg.num_views]
 *   frame_index     device int32 [sum view_counts], each in [0, batch * cfg.num_views) (an entry outside that range yields the black
 *                   view of an empty window, never a read outside `frames`); NULL = the identity: frames / crop_boxes are already
 *                   packed, [sum view_counts] of them
 *   bbox, intrinsic, joints_crop_img, joints_cam, heatmap: PACKED, exactly as for hmv_forward_views
 * HMV_ERR_ARG before anything is launched for whatever hmv_forward_views or hmv_forward_frames refuse.  Always eager, records no stages. */
int hmv_forward_frames_views(hmv_handle h, int32_t batch, const int32_t *view_counts, const uint8_t *frames, int32_t frame_h, int32_t frame_w,
                             const int32_t *crop_boxes, const int32_t *frame_index, const float *mean, const float *std, const float *bbox,
                             const float *intrinsic, float *joints_crop_img, float *joints_cam, float *heatmap, void *stream);

/* The frame preparation alone (op-level parity tests): out_nhwc4 device fp32 [n_frames][out_h][out_w][4] (4th channel 0). */
int hmv_op_prepare_frames(int32_t device, const uint8_t *frames, int32_t n_frames, int32_t frame_h, int32_t frame_w,
                          const int32_t *crop_boxes, const float *mean, const float *std, int32_t out_h, int32_t out_w, float *out_nhwc4,
                          void *stream);

/* ---- occlusion: one patch of one camera's window hidden (the reference's OcclusionAugmentation, datasets/augment.py:102-129) ----
 * The occluder is a rectangle (rx1, ry1, rx2, ry2), int32, in WINDOW pixels: the origin is the window's top-left corner (x1, y1) of the
 * frame's crop box, before the resize; half-open; clipped to [0, cw] x [0, ch] (cw = x2 - x1, ch = y2 - y1).  Window pixels inside it read
 * as 0, exactly like window pixels that fall outside the frame; the filter's weight sums still run over all taps of the window.  The
 * result is, bit for bit, the preparation of the same frame with the frame pixels under the rectangle zeroed.  A rectangle that is empty
 * after clipping (rx2 <= rx1 or ry2 <= ry1) occludes nothing; one that covers the whole window gives the black view of an empty window.
 * The values are untrusted: whatever they are, nothing outside `frames` is read and the work per pixel stays that of the window.
 * The reference's patch (patch_size p, row r, column c; r < ch / p, c < cw / p) is the rectangle (c p, r p, (c + 1) p, (r + 1) p).
 *
 * hmv_op_prepare_frames with one occluder per frame: occ_rects device int32 [n_frames][4]. */
int hmv_op_prepare_frames_occluded(int32_t device, const uint8_t *frames, int32_t n_frames, int32_t frame_h, int32_t frame_w,
                                   const int32_t *crop_boxes, const int32_t *occ_rects, const float *mean, const float *std, int32_t out_h,
                                   int32_t out_w, float *out_nhwc4, void *stream);

/* An occlusion sweep ("which patch of which camera does the prediction rest on"): hmv_forward_frames for the clean batch and for n_occ
 * variants of it, each with one rectangle hidden in ONE camera, at the cost of one per-frame pass over the batch * V clean frames and one
 * occluded frame per (variant, sample) instead of (1 + n_occ) * batch * V frames.  Everything up to the per-frame token rows does not depend
 * on the other views, so a variant reuses the clean rows of its V - 1 untouched cameras; the fusion blocks and the decoder run per variant.
 *   frames, crop_boxes, bbox, intrinsic, joints_crop_img, heatmap: the full clean batch, exactly as for hmv_forward_frames; written once
 *   occ_view             HOST int32 [n_occ], the camera in [0, cfg.num_views) that variant o occludes; read before the call returns
 *   occ_rects            DEVICE int32 [n_occ][batch][4], variant o's rectangle in sample b's window of that camera (see above)
 *   joints_cam           [1 + n_occ][batch][21][3]  out: row 0 the clean batch, row 1 + o variant o
 *   joints_crop_img_occ  [n_occ][batch][21][2]            out, may be NULL: the occluded camera's own 2D output under variant o
 *   heatmap_occ          [n_occ][batch][21][H/8][W/8]     out, may be NULL
 * The rule that defines every number: variant o's joints_cam, joints_crop_img_occ and heatmap_occ hold the bits hmv_forward_frames writes
 * for this batch when, in camera occ_view[o]'s frames, the frame pixels under the rectangle are zeroed; row 0 and the clean outputs hold
 * the bits of hmv_forward_frames on the untouched frames.  A variant's bits depend neither on the passes nor on the other variants;
 * duplicates are allowed.
 * Occluded frame (o, b) is frames[b * V + occ_view[o]] with that slot's window, bbox and intrinsic rows.  The occluded frames go through the
 * per-frame stage in passes of at most max(batch, reserved batch) * V frames, the tail in passes of at most max(batch, reserved batch)
 * virtual samples (one sample under one variant, or clean), so that every buffer of a pass stays within the reservation; the token rows of
 * all batch * V + n_occ * batch frames are retained on top, and the workspace grows before the first launch where that takes it past the
 * reservation.
 * Asynchronous on `stream` and without a device synchronisation (one small table upload).  Always eager, records no stages (reading one
 * afterwards returns HMV_ERR_STATE), ignores attention capture; the range report covers it.  With profiling on, the record list also holds
 * bracketing records "occlusions_frames" (one around the clean stage, one per occluded pass) and "occlusions_tail" (one per tail pass).
 * HMV_ERR_ARG, before anything is launched, for: whatever hmv_forward_frames refuses, n_occ < 1, a NULL occ_view or occ_rects, a camera
 * outside [0, V), (1 + n_occ) * batch beyond the index arithmetic. */
int hmv_forward_frames_occlusions(hmv_handle h, int32_t batch, const uint8_t *frames, int32_t frame_h, int32_t frame_w,
                                  const int32_t *crop_boxes, const float *mean, const float *std, const float *bbox, const float *intrinsic,
                                  int32_t n_occ, const int32_t *occ_view, const int32_t *occ_rects, float *joints_crop_img, float *joints_cam,
                                  float *heatmap, float *joints_crop_img_occ, float *heatmap_occ, void *stream);

/* ---- sequences: the crop window of frame t + 1 is the box around the hand found in frame t ----
 * A recorded or live sequence has no dataset boxes (datasets/ho3d.py:103); its windows follow the hand.  One launch (track.hip) turns a
 * step's joints_crop_img into the next step's windows, per frame slot n (sample, view) with S = float(image_size):
 *   frame-space joints = batch_cropped_joints_to_joints_img (datasets/utils.py:146-162, as handmvnet.py:237 calls it) in its own fp32
 *     operation order, every operation rounded on its own (no fused multiply-add):
 *       X = fl(fl(u * fl(fl(float(x2) - float(x1)) / S)) + float(x1)),  Y likewise with y1, y2
 *   next window = points2d_to_bbox(points, margin, square) (datasets/utils.py:5-27) exactly: minimum / maximum over the 21 joints truncated
 *     toward zero (Python's int()), the shorter side of a `square` box widened by |h - w| (the odd pixel goes to the low edge), then margin.
 *   joints_crop_img [n_slots][21][2] fp32, crop pixels as a forward returns them;  crop_boxes_in [n_slots][4] int32 = x1, y1, x2, y2
 *   present         device uint8 [n_slots] or NULL (= every slot present)
 *   crop_boxes_out  [n_slots][4] int32;  bbox_out [n_slots][4] fp32 or NULL: the same four numbers as fp32 (what hmv_forward_frames takes as bbox)
 *   joints_img      [n_slots][21][2] fp32 or NULL: the frame-space joints;  status [n_slots] int32 or NULL
 * status 0: the window moved.
 * status 1: present[n] == 0.  Window copied through (bbox_out = its fp32), joints_img row zeros (hmv_forward_views' callers zero an absent
 *           view's joints: followed blindly they would collapse the window onto the crop corner).
 * status 2: one of the 42 frame-space coordinates is non-finite or has magnitude >= 1e9 (int conversion would overflow), or the new window
 *           would be wider or taller than 65536 px (which hmv_forward_frames reads as the black view).  Window copied through (bbox_out =
 *           its fp32), joints_img as computed.  The reference raises here; device code cannot, so it reports.
 * An empty input window (x2 <= x1 or y2 <= y1) is not special: the arithmetic is defined for it and is the reference's.
 * crop_boxes_out may be crop_boxes_in and bbox_out may alias any fp32 copy of it: a slot reads its window before it writes, and no slot
 * reads another's.  Takes no handle; asynchronous on `stream`.  HMV_ERR_ARG before any launch (hmv_last_error(NULL) names it) for
 * n_slots <= 0, image_size <= 0, margin < 0, a NULL joints_crop_img / crop_boxes_in / crop_boxes_out. */
int hmv_op_next_crop_boxes(int32_t device, int32_t n_slots, const float *joints_crop_img, const int32_t *crop_boxes_in, const uint8_t *present,
                           int32_t image_size, int32_t margin, int32_t square, int32_t *crop_boxes_out, float *bbox_out, float *joints_img,
                           int32_t *status, void *stream);

/* hmv_forward_frames, then on the same stream hmv_op_next_crop_boxes (image_size = cfg.image_size, every slot present) from the
 * joints_crop_img just written, IN PLACE: crop_boxes [batch*V][4] becomes the next step's windows and bbox (when not NULL: no 'crop' in
 * pos_enc needs none) their fp32.  joints_img [batch*V][21][2] and status [batch*V] as above, each may be NULL.  A sequence is this one call
 * per time step on unchanged buffers: nothing crosses to the host.
 * Takes part in graph replay exactly like hmv_forward_frames, tracking launch included; the key also covers joints_img, status, margin
 * and square (a call is never served by a graph of hmv_forward_frames or the other way round).  Stage capture and profiling force the
 * eager path.  hmv_launch_count counts the extra launch.  HMV_ERR_ARG before any launch for margin < 0 and whatever hmv_forward_frames refuses. */
int hmv_forward_frames_track(hmv_handle h, int32_t batch, const uint8_t *frames, int32_t frame_h, int32_t frame_w, int32_t *crop_boxes,
                             const float *mean, const float *std, float *bbox, const float *intrinsic, float *joints_crop_img,
                             float *joints_cam, float *heatmap, int32_t margin, int32_t square, float *joints_img, int32_t *status,
                             void *stream);

/* The same tail behind hmv_forward_frames_views; always eager and records no stages, as that entry.
 *   crop_boxes   stays in the caller's FULL [batch * cfg.num_views] layout and is updated in place: packed row n (its joints_crop_img row)
 *                moves the window of slot frame_index[n].  A slot is present iff some packed frame names it; the window of an absent slot
 *                is left alone.  The entries of frame_index must be distinct (two rows naming one slot race for its window); an entry
 *                outside the range moves nothing.
 *   bbox         PACKED, as in that entry: row n receives the fp32 of its slot's new window (NULL: not updated)
 *   joints_img [batch * cfg.num_views][21][2], status [batch * cfg.num_views]: FULL layout, each may be NULL; an absent slot reads status 1
 *                and zero joints (two fills in front of the tracking launch).
 * frame_index == NULL (frames and windows already packed): the layout is the packed one, [sum view_counts] slots, all present. */
int hmv_forward_frames_views_track(hmv_handle h, int32_t batch, const int32_t *view_counts, const uint8_t *frames, int32_t frame_h,
                                   int32_t frame_w, int32_t *crop_boxes, const int32_t *frame_index, const float *mean, const float *std,
                                   float *bbox, const float *intrinsic, float *joints_crop_img, float *joints_cam, float *heatmap,
                                   int32_t margin, int32_t square, float *joints_img, int32_t *status, void *stream);

/* Evaluation metrics of HandMvNet._get_metrics (handmvnet.py:352-368) on the device, replacing
 * PoseMetrics.mpjpe / pa_mpjpe / pck / pck_auc / compute_similarity_transform (models/metrics.py:6-24, 64-176).
 * pred, target: device fp32 [n_sets][n_pts][dim] (dim 2 or 3; units as given -- the caller applies the x1000 the
 * reference applies).  Thresholds = torch.linspace(thr_min, thr_max, steps), 1 <= steps <= 256.
 * procrustes != 0 (dim == 3 only): also the similarity-aligned error; aligned (device [n_sets][n_pts][3] or NULL)
 * receives the aligned predictions.  result: device fp32 [4 + 2*steps] =
 *   { mpjpe, pa_mpjpe (NaN if not requested), auc, norm_auc, pck[steps], thresholds[steps] }.
 * Asynchronous on `stream`; one single-workgroup launch with fixed-order reductions (bit-reproducible). */
int hmv_pose_metrics(int32_t device, const float *pred, const float *target, int32_t n_sets, int32_t n_pts, int32_t dim,
                     float thr_min, float thr_max, int32_t steps, int32_t procrustes, float *aligned, float *result,
                     void *stream);

/* ---- evaluation-step losses (HandMvNet._calculate_loss, handmvnet.py:279-351) ----
 * Stateless like the metrics entry: a device ordinal and a stream, asynchronous, device pointers throughout.  A bad argument returns
 * HMV_ERR_ARG and the text behind a NULL handle's last error names it.  Sums are fp64 and every reduction has a fixed order, so
 * results are bit-reproducible; per-element arithmetic is fp64 where the reference's is fp32 (parity is stated against the
 * reference evaluated in float64).
 *
 * Three behaviours of the reference are worth knowing:
 *   - a label whose whole Gaussian lies outside the image (truncated coordinate c >= S + 3 sigma or c <= -3 sigma - 2 on either
 *     axis): the reference's generate_heatmap returns a tuple there (datasets/utils.py:105) and the dataset transform raises; this
 *     library writes the all-zero map that line's comment intends (c = -3 sigma - 1 is an all-zero map in the reference too);
 *   - the crop mapping of the reprojection always scales by 256: handmvnet.py:332 passes no image_size, so datasets/utils.py:128-129
 *     uses its default even for a 128-pixel configuration.  Reproduced as is;
 *   - a singular extrinsic makes torch.inverse raise; a kernel cannot, so the coordinates (and the terms built on them) come out
 *     non-finite. */

/* The dataset's ground-truth heat maps (datasets/ho3d.py:155-166): per joint generate_heatmap on a zero image_size x image_size image
 * (datasets/utils.py:86-121; the label truncated toward zero, 6 sigma + 1 taps exp(-d^2 / (2 sigma^2)) per axis, cropped to the image)
 * -> ToTensor in float64 -> Resize((hm_h, hm_w), antialias=True) -> fp32.  Evaluated separably in fp64 (row profile x column profile,
 * one rounding), which matches the reference's float64 pipeline to the last fp32 bit or the one next to it.
 *   joints [n_frames][21][2] crop-image x, y;  out [n_frames][21][hm_h][hm_w];  sigma an integer in 1 .. 8 (the reference uses 2);
 *   hm_h, hm_w >= 1 with hm_h + hm_w <= 256, independent of each other and of image_size (the scales need not be integers). */
int hmv_op_target_heatmaps(int32_t device, const float *joints, int32_t n_frames, int32_t image_size, int32_t hm_h, int32_t hm_w,
                           int32_t sigma, float *out, void *stream);

/* get_2d_joints_from_3d_joints (utils/camera.py:25-44) as one launch instead of a Python loop over batch x views:
 *   X_w = extrinsic[b][root_idx] [X; 1],  X_i = inverse(extrinsic[b][i]) X_w  (a GENERAL 4x4 inverse in fp64, as torch.inverse is:
 *   not [R^T | -R^T t]),  x1000,  u = x fx / (z + 1e-6) + cx,  v = y fy / (z + 1e-6) + cy.
 *   joints_abs [B][21][3] metres in camera root_idx;  extrinsic [B][V][4][4];  intrinsic [B][V][4] = fx, fy, cx, cy;
 *   bbox NULL: out [B][V][21][2] in image pixels (what the reference function returns);
 *   bbox [B][V][4] = x1, y1, x2, y2: followed by batch_joints_img_to_cropped_joints, (u - x1) 256 / (x2 - x1), (v - y1) 256 / (y2 - y1). */
int hmv_project_joints(int32_t device, const float *joints_abs, int32_t B, int32_t V, int32_t root_idx, const float *intrinsic,
                       const float *extrinsic, const float *bbox, float *out, void *stream);

typedef struct hmv_loss_args {
    int32_t struct_size;            /* sizeof(hmv_loss_args), ABI guard */
    int32_t B, V;                   /* samples, views */
    int32_t hm_h, hm_w;             /* size of the predicted heat maps */
    int32_t image_size, sigma;      /* read when target_heatmap is NULL: the S and sigma of hmv_op_target_heatmaps */
    int32_t root_idx;               /* inputs["root_idx"][0]: the camera joints_cam + root_joint live in (with_projection) */
    int32_t mask_invisible_joints;  /* train_params["mask_invisible_joints"] */
    int32_t with_projection;        /* "g2d" in train_params["loss_weights"]: the g2d / p2d terms exist */
    float w_heatmap, w_joints_2d, w_joints_3d, w_g2d, w_p2d;   /* train_params["loss_weights"] */
    int32_t reserved;               /* 0 */
    const float *pred_heatmap;      /* out["heatmap"]            [B][V][21][hm_h][hm_w] */
    const float *target_heatmap;    /* inputs["heatmap"], same shape; NULL: synthesised per joint from gt_joints_2d exactly as
                                     * hmv_op_target_heatmaps would (same device function: the two forms give the same bits) */
    const float *pred_joints_2d;    /* out["joints_crop_img"]    [B][V][21][2] */
    const float *gt_joints_2d;      /* inputs["joints_crop_img"] [B][V][21][2] */
    const uint8_t *joints_mask;     /* inputs["joints_img_mask"] [B][V][21], non-zero = invisible; may be NULL */
    const float *pred_joints_cam;   /* out["joints_cam"]         [B][21][3] metres, root-relative */
    const float *gt_joints_cam;     /* inputs["joints_cam"]      [B][21][3] metres */
    const float *root_joint;        /* inputs["root_joint"]      [B][3] metres; NULL = zeros (with_projection) */
    const float *intrinsic;         /* [B][V][4]     (with_projection) */
    const float *extrinsic;         /* [B][V][4][4]  (with_projection) */
    const float *bbox;              /* [B][V][4]     (with_projection) */
    float *projected;               /* out["projected_joints_crop_img"] [B][V][21][2], optional output (with_projection) */
    void *scratch;                  /* caller-owned device buffer, 8-byte aligned */
    size_t scratch_bytes;           /* >= what the scratch sizing entry below gives for B, V */
} hmv_loss_args;

/* Bytes of scratch one loss call over B samples of V views needs (one fp64 partial per frame). */
size_t hmv_pose_losses_scratch_bytes(int32_t B, int32_t V);

/* Every term of _calculate_loss for a root-relative model.  result: device fp32 [6] =
 *   { heatmap_loss, joints_2d_loss, joints_3d_loss, g2d_loss, p2d_loss, loss }   (root_3d_loss is the constant 0; [3], [4] are 0 without
 *   with_projection; loss is the sum of the terms present)
 *   heatmap_loss   = w_heatmap   * mean (pred - target)^2 over [B][V][21][hm_h][hm_w]
 *   joints_2d_loss = w_joints_2d * mean |p - g| over [B][V][21][2]; with a mask AND mask_invisible_joints, masked joints are zeroed
 *                    on both sides and the divisor stays the full count (models/utils.py:123-131)
 *   joints_3d_loss = w_joints_3d * mean |pred_joints_cam - gt_joints_cam|
 *   g2d_loss / p2d_loss = w * mean |proj - gt_joints_2d| / |proj - pred_joints_2d|, unmasked like the reference; proj is the crop-mapped
 *                    projection of pred_joints_cam + root_joint (the projection entry above with a bbox), used at fp64 before the
 *                    rounding that `projected` receives.
 * Two launches: one workgroup per frame writes the fp64 sum of its 21 * hm_h * hm_w squared differences to scratch (16-byte loads
 * where the frame's base addresses allow, scalar loads otherwise, added in the same order either way); one workgroup then adds the
 * frame sums in index order and computes the small terms.  The bits depend on neither the number of workgroups in flight, nor
 * alignment, nor the target form. */
int hmv_pose_losses(int32_t device, const hmv_loss_args *args, float *result, void *stream);

/* hmv_pose_losses for a RAGGED view set (hmv_forward_views): view_present is a device uint8 [B][V], non-zero = the view is present.
 * Same struct (size and layout), the same [B][V] tensor layout, scratch sizing and result vector.  The rule: the value of every term is
 * the mean, over the batch's samples, of the value the reference logs for that sample alone (batch 1) over its present views P_b only
 * (v_b = |P_b|) -- what hmv_forward_views computes for the sample, and independent of how a split is cut into batches:
 *   heatmap_loss        = w * 1/B sum_b [ sum_{v in P_b} sum (pred - target)^2 / (v_b * 21 * hm_h * hm_w) ]
 *   joints_2d_loss      = w * 1/B sum_b [ sum_{v in P_b} sum |p keep - g keep| / (v_b * 42) ]      (keep: the uniform entry's mask rule)
 *   g2d_loss / p2d_loss = w * 1/B sum_b [ sum_{v in P_b} sum |proj - g| / (v_b * 42) ],  |proj - p| likewise
 *   joints_3d_loss has no view axis and is the uniform entry's; loss is the sum of the terms.
 * intrinsic, extrinsic and bbox stay FULL [B][V] tables and root_idx indexes the full table: calibration is known for a camera whose
 * frame is absent, so the root camera may itself be absent.  An absent slot contributes nothing whatever its rows hold (zeros from
 * hmv_forward_views, garbage, NaN): its maps, joints and joint-mask row are not read, and no target map is synthesised for it.
 * `projected` receives the projection for present slots and zeros for absent ones.  With every view present the result has the bits
 * of hmv_pose_losses.  view_present == NULL is HMV_ERR_ARG (the uniform entry is the one for that); the other checks are the uniform
 * entry's, in front of every HIP call.
 * PRECONDITION: every sample has at least one present view (hmv_forward_views refuses a batch that breaks it).  The mask is device
 * data and cannot be checked without a synchronisation, so it is not: a sample without a view causes no out-of-bounds access and
 * makes the view-dependent terms (and loss) NaN.
 * Two launches like the uniform entry: one workgroup per frame slot (that of an absent slot writes 0 and leaves at once), then one
 * workgroup that derives v_b from the mask rows and applies the per-sample divisors. */
int hmv_pose_losses_views(int32_t device, const hmv_loss_args *args, const uint8_t *view_present, float *result, void *stream);

/* ---- evaluation epoch (what trainer.validate / trainer.test hand back: one set of numbers for the whole split) ----
 * hmv_eval_add adds one evaluation step -- everything HandMvNet._calculate_mpjpe (handmvnet.py:370-427) computes for it, and the loss
 * vector the loss entry above wrote -- into a caller-owned fp64 state vector in device memory.  Nothing is copied to the host: the
 * caller reads the state back once per epoch and divides.  The epoch value of every quantity is
 *     sum over steps (and ranks) of B x the step's value  /  sum of B,
 * the batch-size-weighted mean that Lightning's on_epoch logging produces; MPJPE, PA-MPJPE, 2D MPJPE and the PCK curve are linear in
 * the rows, so for them it is the value on the pooled split, whatever the cut into batches and ranks.
 *
 * State layout: a contiguous array of 15 + steps doubles (hmv_eval_state_doubles(steps)):
 *   [0]   samples, sum of B                          [1]   steps added
 *   [2]   3D rows, sum of B * 21                     [3]   sum of the 3D joint distances (the units of joints_cam: metres)
 *   [4]   sum of the distances after the per-pose similarity alignment
 *   [5]   2D rows, sum of B * V * 21                 [6]   sum of the 2D joint distances (crop-image pixels)
 *         (a ragged step, hmv_eval_add_views, counts rows in units of a FULL sample: [5] still grows by B * V * 21, and each present
 *         row of sample b adds its distance times V / v_b to [6], so that [6] / [5] stays the mean over samples of each sample's own 2D
 *         MPJPE over its v_b present views; the factor is exactly 1.0 for a full sample)
 *   [7]   sum of B over the steps that carried a loss
 *   [8 .. 13]   sum of B * term for the six values of the loss vector, in its order
 *               { heatmap_loss, joints_2d_loss, joints_3d_loss, g2d_loss, p2d_loss, loss }
 *   [14 .. 14 + steps]   PCK histogram of the 3D distances, steps + 1 bins: bin i counts the rows whose first threshold with
 *               dist <= thr is thr[i], thr = torch.linspace(thr_min, thr_max, steps) in fp32; the last bin the rows beyond thr_max.
 *               The PCK curve is the cumulative histogram over [2].
 * Counts are integers held in doubles (exact below 2^53).  A masked joint (joints_mask non-zero) is zeroed on both sides, as
 * models/utils.py:123-131 does: it adds the distance 0 and still counts in [5].  A zero-filled buffer is an empty epoch, so there is
 * no reset entry; summing the states of several ranks element by element gives the state of their union.
 * The state belongs to one stream at a time: stream order is what orders successive steps (the kernel's final read-modify-write of the
 * state is done by one thread, without atomics).
 *
 * One single-workgroup launch with the per-row arithmetic of the metrics entry above (same device functions): fp32 for the distance
 * versus threshold comparison, fp64 sums in a fixed order and the 3x3 Procrustes problem in fp64, no floating-point atomics -- two
 * identical epochs give identical bits. */
typedef struct hmv_eval_args {
    int32_t struct_size;            /* sizeof(hmv_eval_args), ABI guard */
    int32_t B, V;                   /* samples, views */
    int32_t steps;                  /* PCK thresholds, 1 .. 256 (the reference uses 20) */
    float thr_min, thr_max;         /* thr_min <= thr_max, the units of joints_cam */
    const float *pred_joints_cam;   /* out["joints_cam"]         [B][21][3] metres */
    const float *gt_joints_cam;     /* inputs["joints_cam"]      [B][21][3] metres */
    const float *pred_joints_2d;    /* out["joints_crop_img"]    [B][V][21][2] */
    const float *gt_joints_2d;      /* inputs["joints_crop_img"] [B][V][21][2] */
    const uint8_t *joints_mask;     /* inputs["joints_img_mask"] [B][V][21], non-zero = invisible; may be NULL */
    const float *loss_result;       /* the device float[6] the loss entry wrote for this step; NULL: a step without loss labels */
    double *state;                  /* device, 8-byte aligned */
    size_t state_doubles;           /* >= hmv_eval_state_doubles(steps) */
} hmv_eval_args;

/* Doubles in the state of an epoch with `steps` thresholds: 15 + steps; 0 when steps is outside 1 .. 256. */
size_t hmv_eval_state_doubles(int32_t steps);

/* Adds one step to args->state, asynchronously on `stream`.  Every argument is checked before any HIP call: a bad one returns
 * HMV_ERR_ARG and the text behind a NULL handle's last error names it. */
int hmv_eval_add(int32_t device, const hmv_eval_args *args, void *stream);

/* hmv_eval_add for one step of a RAGGED view set: view_present as for hmv_pose_losses_views (device uint8 [B][V], every sample with at
 * least one present view; NULL is HMV_ERR_ARG), loss_result the vector that entry wrote.  Same struct, state and layout; one
 * single-workgroup launch.  Everything but the 2D sum is what hmv_eval_add adds; for [5] / [6] see the state layout.  The rows of absent
 * views are not read (nor their joint mask).  The rows are walked in hmv_eval_add's order: with every view present the state has its
 * bits, and ragged and uniform steps may be mixed in one epoch. */
int hmv_eval_add_views(int32_t device, const hmv_eval_args *args, const uint8_t *view_present, void *stream);

/* ---- evaluation breakdown (the epoch's errors kept apart by joint, by camera and by sample) ----
 * hmv_eval_breakdown_add adds the step that hmv_eval_add / hmv_eval_add_views pooled -- same tensors, same stream -- into a SECOND
 * caller-owned fp64 state, and optionally writes one fp32 record row per sample.  The pooled state and its entries are untouched by
 * it.  Every number is the reference's PoseMetrics.mpjpe / compute_similarity_transform / pck / mask_joints applied to one joint
 * column or one camera slice.
 *
 * State layout: hmv_eval_breakdown_doubles(V, steps) = 4 + 42 + 21 (S + 1) + 43 V doubles, S = steps, every slice a sum over the
 * steps added:
 *   [0]   samples, sum of B            [1]   steps added
 *   [2]   V        [3]   S             written by the first add (the one that finds [1] == 0), not added to afterwards: a state is
 *                                      additive only with one of the same V and S, and whoever sums two states keeps [2] and [3]
 *   J3  [21]          per joint: sum over samples of the fp32 3D distance (metres)
 *   JPA [21]          per joint: sum of the distance that remains after the pose's similarity alignment (the fp64 arithmetic of [4]
 *                     of the pooled state)
 *   H   [21][S + 1]   per joint: the PCK histogram bins of the pooled state's [14 ..], integer-valued; summed over the joints they
 *                     are that histogram
 *   CN  [V]           per camera: samples in which it is present
 *   C2  [V][21]       per camera and joint: sum over its present slots of the 2D distance, a masked joint zeroed on both sides and
 *                     adding 0 (the pooled state's rule for [6])
 *   CV  [V][21]       per camera and joint: present slots in which the joint is NOT masked; CN[v] without a joint mask
 * C2[v] / CN[v] is the camera's 2D MPJPE under the masking rule, C2[v][j] / CV[v][j] the error over the visible joints alone.
 * A ragged step (view_present not NULL) adds each PRESENT slot unweighted and does not read an absent one: the value of a camera is
 * the one over the samples that had this camera.  That is deliberately not the V / v_b weighting of the pooled [6], which is a mean
 * over samples; the sum of C2 equals [6] only for steps with every view.
 *
 * Record row of sample b: hmv_eval_record_floats(V) = 4 + V floats at records[(record_base + b) * (4 + V)]
 *   [0]   the mean of its 21 fp32 3D distances (metres)      [1]   that mean after its similarity alignment
 *   [2]   its 2D MPJPE over its present views and 21 joints under the masking rule (the per-sample value of the ragged convention);
 *         NaN for a sample without a present view, which is a broken precondition as for hmv_eval_add_views -- nothing is indexed
 *         by a count
 *   [3]   v_b, its present views
 *   [4 + v]   camera v's 2D error over the 21 joints; NaN when the camera is absent
 * each the fp64 mean of fp32 distances, rounded to fp32 once.  The caller counts samples on the host and passes the row of this
 * step's sample 0, so nothing is read back to place a row; rows outside record_base .. record_base + B - 1 are not touched.
 *
 * One launch of 2 + V workgroups (3 + V with records), each the only writer of its slice: fp32 where the reference compares, fp64
 * sums and Procrustes, every sum in a fixed order, no floating-point atomics -- two identical epochs give identical bits in state and
 * records.  Like the pooled state, this one belongs to one stream at a time, and a zero-filled buffer is an empty epoch.  The V of a
 * later step cannot be compared with [2] without a synchronisation, so it is not: the caller keeps V and steps the same. */
typedef struct hmv_eval_breakdown_args {
    int32_t struct_size;            /* sizeof(hmv_eval_breakdown_args), ABI guard */
    int32_t B, V;                   /* samples, views */
    int32_t steps;                  /* PCK thresholds, 1 .. 256 */
    float thr_min, thr_max;         /* thr_min <= thr_max, the units of joints_cam */
    const float *pred_joints_cam;   /* as in hmv_eval_args, all five */
    const float *gt_joints_cam;
    const float *pred_joints_2d;
    const float *gt_joints_2d;
    const uint8_t *joints_mask;     /* may be NULL */
    const uint8_t *view_present;    /* device uint8 [B][V], non-zero = the view is there; NULL: every view is present */
    double *state;                  /* device, 8-byte aligned */
    size_t state_doubles;           /* >= hmv_eval_breakdown_doubles(V, steps) */
    float *records;                 /* device fp32 [record_capacity][4 + V]; may be NULL: no records, the next two are ignored */
    int64_t record_capacity;        /* rows */
    int64_t record_base;            /* the row of this step's sample 0 */
} hmv_eval_breakdown_args;

/* Doubles in a breakdown state: 4 + 42 + 21 (steps + 1) + 43 V (831 for V = 8, steps = 20); 0 for V < 1 or steps outside 1 .. 256. */
size_t hmv_eval_breakdown_doubles(int32_t V, int32_t steps);

/* Floats in one record row: 4 + V; 0 for V < 1. */
size_t hmv_eval_record_floats(int32_t V);

/* Adds one step, asynchronously on `stream`.  Every argument is checked before any HIP call, with hmv_eval_add's rules and texts;
 * further HMV_ERR_ARG, with nothing launched: state_doubles too small, and with records a misaligned pointer, record_capacity < 1,
 * record_base < 0 or a last sample that would land at record_base + B > record_capacity. */
int hmv_eval_breakdown_add(int32_t device, const hmv_eval_breakdown_args *args, void *stream);

/* ---- absolute evaluation (where the hand is, over a whole split: the world MPJPE, and what the triangulation says about the rig) ----
 * hmv_eval_absolute_add adds one step of HandMvNet.forward_absolute -- the root-relative prediction, the triangulated joints with
 * their status, and optionally the triangulation launch's reprojection errors and inlier counts (hmv_op_triangulate's points3d with a
 * frame_cam, status, reproj_err, inliers) -- into a THIRD caller-owned fp64 state.  The pooled and the breakdown state are untouched by
 * it.  The labels must be in the frame joints_tri is in: each sample's reference camera, view 0 or a ragged sample's first present
 * view.
 *
 * A sample is LOCATED when tri_status[b][0] == 0 and the three coordinates of joints_tri[b][0] are finite; every other sample is
 * LOST and adds to [0] and to S, TN, R, H only.  The world distance of (b, j) is
 *     | (pred_joints_cam[b][j] + joints_tri[b][0])  -  (gt_joints_cam[b][j] + gt_root[b]) |
 * with both sums rounded to fp32 (what the evaluation step computes for {mode}_w_mpjpe, handmvnet.py:412-413) and the fp32 joint
 * distance of the other evaluation entries.
 *
 * State layout: hmv_eval_absolute_doubles(V) = 156 + 3 V doubles, additive element by element except [2]:
 *   [0]   samples, sum of B            [1]   steps added
 *   [2]   V: WRITTEN by every add, not summed.  An add whose V differs from a non-zero [2] is refused; whoever sums two states
 *         (an all-reduce) refills it
 *   [3]   located samples
 *   [4]   sum over the located samples and their 21 joints of the world distance (the units of joints_cam: metres)
 *   [5]   sum over the located samples of | joints_tri[b][0] - gt_root[b] |
 *   [6], [7]   reserved, left as they are
 *   W   [21]      at [8]:   per joint, the world distance summed over the located samples; [4] is the sum of this step's 21 values
 *   T   [21]      at [29]:  per joint, sum of | joints_tri[b][j] - (gt_joints_cam[b][j] + gt_root[b]) | over the samples with
 *                           tri_status[b][j] == 0 and a finite point: plain triangulation against the labels
 *   TN  [21]      at [50]:  the count for T
 *   S   [21][4]   at [71]:  per joint, the samples whose tri_status[b][j] is 0, 1, 2, 3; a value outside 0 .. 3 counts as 3
 *   R   [V]       at [155]:       per camera, sum of the finite reproj_err[b][v][j] over the (b, j) with status 0 (pixels)
 *   RN  [V]       at [155 + V]:   the count for R.  R and RN are untouched when reproj_err is NULL
 *   H   [V + 1]   at [155 + 2 V]: the (b, j) with status 0 whose inliers value, clamped to 0 .. V, is k.  Untouched when inliers is NULL
 * Counts are integers held in doubles.  A zero-filled buffer is an empty epoch.
 *
 * One launch of 2 to 4 workgroups, each the only writer of its slice and each element read-modify-written by one lane: fp32
 * distances, fp64 sums in a fixed order, no floating-point atomics -- two identical epochs give identical bits.  The loops stride over
 * the B * 21 rows and the B * V * 21 reprojection entries.  The kernel reports and repairs nothing: a non-finite label or prediction of
 * a located sample makes its distance non-finite, and that distance goes into [4], [5], W or T as it is.
 * The state belongs to one stream at a time.  To compare V with [2] the entry reads those eight bytes back behind the stream's
 * earlier work before it launches: unlike hmv_eval_add it waits for the stream once per call.  A caller that keeps the epoch's V on
 * the host and has compared there sets v_checked: nothing is read back and nothing waits.  The kernel compares as well, in either
 * case: on a state begun with another V it writes nothing, so a wrong promise loses the step and not the epoch. */
typedef struct hmv_eval_absolute_args {
    int32_t struct_size;            /* sizeof(hmv_eval_absolute_args), ABI guard */
    int32_t B, V;                   /* samples; views, 1 .. 16 as for hmv_op_triangulate */
    int32_t v_checked;              /* 0: the entry compares V with state[2] (one wait for the stream); non-zero: the caller has */
    const float *pred_joints_cam;   /* out["joints_cam"]      [B][21][3] metres */
    const float *joints_tri;        /* out["joints_tri"]      [B][21][3] in each sample's reference-camera frame */
    const int32_t *tri_status;      /* out["tri_status"]      [B][21] */
    const float *gt_joints_cam;     /* inputs["joints_cam"]   [B][21][3] metres */
    const float *gt_root;           /* inputs["root_joint"]   [B][3] metres */
    const float *reproj_err;        /* the triangulation's reproj_err [B][V][21]; may be NULL */
    const int32_t *inliers;         /* the triangulation's inliers [B][21]; may be NULL */
    double *state;                  /* device, 8-byte aligned */
    size_t state_doubles;           /* >= hmv_eval_absolute_doubles(V) */
} hmv_eval_absolute_args;

/* Doubles in an absolute state: 156 + 3 V (180 for V = 8); 0 for V outside 1 .. 16. */
size_t hmv_eval_absolute_doubles(int32_t V);

/* Adds one step on `stream`.  Every argument is checked before any HIP call: a NULL args, a struct_size other than
 * sizeof(hmv_eval_absolute_args), B < 1, V outside 1 .. 16, B * V beyond 2^24, a NULL pred_joints_cam / joints_tri / tri_status /
 * gt_joints_cam / gt_root, a NULL or misaligned state, or a state_doubles below hmv_eval_absolute_doubles(V) returns HMV_ERR_ARG and
 * the text behind a NULL handle's last error names the field.  So does, with v_checked == 0, a V that differs from a non-zero
 * state[2]; nothing is launched then and the state keeps its bytes. */
int hmv_eval_absolute_add(int32_t device, const hmv_eval_absolute_args *args, void *stream);

/* ---- vertex evaluation (the mesh block of _calculate_mpjpe over a whole split: MPVPE, PA-MPVPE, the vertex PCK curve) ----
 * hmv_eval_vertices_add adds one step's predicted and labelled meshes -- what HandMvNet._calculate_mpjpe (handmvnet.py:389-408) hands
 * to PoseMetrics as `vertices / 1000.` -- into a FOURTH caller-owned fp64 state, and optionally writes one fp32 record row per sample.
 * The other states and their entries are untouched by it.  Every number is the reference's PoseMetrics.mpjpe /
 * compute_similarity_transform / pck applied to [B][n_verts][3] point sets.
 *
 * A sample whose status is non-zero (hmv_op_hand_ik's or hmv_op_mano_skin's status of the row that made its mesh) is SKIPPED: its
 * vertices are not read, it adds to [4] only, and its record row is NaN.  With status == NULL every sample is added, and a mesh
 * with a NaN then makes the sums NaN, as it does in the reference.
 *
 * State layout: hmv_eval_vertices_doubles(n_verts, steps) = 8 + (S + 1) + 2 n_verts doubles, S = steps, additive element by element
 * except [2] and [3]:
 *   [0]   samples added (status 0)      [1]   steps added
 *   [2]   n_verts      [3]   S          written by the first add (the one that finds [1] == 0), not added to afterwards, like [2]
 *                                       and [3] of the breakdown state: whoever sums two states keeps them
 *   [4]   samples skipped               [5]   vertex rows, [0] * n_verts
 *   [6]   sum of the fp32 vertex distances (the units after unit_div: metres for millimetres and unit_div = 1000)
 *   [7]   sum of the distances that remain after each mesh's similarity alignment (fp64)
 *   H   [S + 1]     at [8]:  the PCK histogram of the fp32 distances, the bins of hmv_eval_add's [14 ..]; it sums to [5]
 *   PV  [n_verts]   per vertex: sum over the added samples of its fp32 distance
 *   PVA [n_verts]   per vertex: the same after the alignment
 * [6] / [5] is the MPVPE, [7] / [5] the PA-MPVPE, the cumulative H over [5] the curve {mode}_pck_v.  Counts are integers held in
 * doubles.  A zero-filled buffer is an empty epoch.
 *
 * Record row of sample b: two floats at records[(record_base + b) * 2]
 *   [0]   the mean of its n_verts fp32 distances      [1]   that mean after its alignment
 * each an fp64 mean rounded to fp32 once; both NaN for a skipped sample.  The caller counts samples on the host and passes the row of
 * this step's sample 0, as for hmv_eval_breakdown_add.
 *
 * Both meshes are divided by unit_div first, every coordinate in fp32 and correctly rounded (the reference's `vertices / 1000.`);
 * the distance is the fp32 one of the joint entries, the alignment their fp64 arithmetic on centred values.
 *
 * Two launches.  The first runs one workgroup per sample, all of whose lanes walk that sample's vertices: the meshes are staged in
 * LDS once and read three times, one lane solves the 3x3 problem in between.  It leaves every vertex's two distances and the
 * sample's partial sums in `scratch`.  The second, 1 + ceil(n_verts / 256) workgroups each the only writer of its slice, adds them
 * onto the state one sample after the other in row order.  Every sum has a fixed order and there are no floating-point atomics; a
 * sample's values depend neither on B nor on its row.  So two identical epochs give identical bits, and so do two epochs that cut
 * the same samples, in the same order, into different batches -- in everything but [1], which counts the adds.
 * The state belongs to one stream at a time, and the scratch to this call: it may be reused by the next call on the same stream.
 * n_verts and steps of a later step cannot be compared with [2] and [3] without a synchronisation, so they are not: the caller keeps
 * them the same. */
typedef struct hmv_eval_vertices_args {
    int32_t struct_size;            /* sizeof(hmv_eval_vertices_args), ABI guard */
    int32_t B, n_verts;             /* samples, 1 .. 4096; vertices of a mesh, 1 .. 4096 (MANO: 778) */
    int32_t steps;                  /* PCK thresholds, 1 .. 256 (the reference uses 20) */
    float thr_min, thr_max;         /* thr_min <= thr_max, in the units AFTER unit_div */
    float unit_div;                 /* finite and > 0; 1.0f leaves the coordinates alone */
    const float *pred_vertices;     /* out["vertices"]    [B][n_verts][3] */
    const float *gt_vertices;       /* inputs["vertices"] [B][n_verts][3] */
    const int32_t *status;          /* device int32 [B]; may be NULL: every sample is added */
    double *state;                  /* device, 8-byte aligned */
    size_t state_doubles;           /* >= hmv_eval_vertices_doubles(n_verts, steps) */
    void *scratch;                  /* device, 8-byte aligned; written by the call, nothing of it is kept */
    size_t scratch_bytes;           /* >= hmv_eval_vertices_scratch_bytes(B, n_verts, steps) */
    float *records;                 /* device fp32 [record_capacity][2]; may be NULL: no records, the next two are ignored */
    int64_t record_capacity;        /* rows */
    int64_t record_base;            /* the row of this step's sample 0 */
} hmv_eval_vertices_args;

/* Doubles in a vertex state: 8 + (steps + 1) + 2 n_verts (1585 for 778 vertices and 20 thresholds); 0 for n_verts outside 1 .. 4096
 * or steps outside 1 .. 256. */
size_t hmv_eval_vertices_doubles(int32_t n_verts, int32_t steps);

/* Bytes of scratch one call takes: B (8 (steps + 4) + 12 n_verts); 0 for a B or n_verts outside 1 .. 4096 or steps outside 1 .. 256. */
size_t hmv_eval_vertices_scratch_bytes(int32_t B, int32_t n_verts, int32_t steps);

/* Adds one step, asynchronously on `stream`.  Every argument is checked before any HIP call, with hmv_eval_add's texts where the rule
 * is the same: a NULL args, a wrong struct_size, B, n_verts or steps out of range, thr_max below thr_min, a unit_div that is not
 * finite and > 0, a NULL pred_vertices / gt_vertices, a misaligned status, a NULL or misaligned state or scratch, a state_doubles or
 * scratch_bytes below what the two functions above give, and with records hmv_eval_breakdown_add's rules for them return
 * HMV_ERR_ARG with nothing launched. */
int hmv_eval_vertices_add(int32_t device, const hmv_eval_vertices_args *args, void *stream);

/* ---- sequence evaluation (a followed sequence, hmv_forward_frames_track: labels in the tracker's windows, jitter, window quality) ----
 * Under a tracker the windows are the tracker's own, so 2D labels expressed in dataset boxes do not belong to the predictions.  The
 * three entries below keep the evaluation of such a sequence on the device.  Stateless like the metrics, loss and track entries: a
 * device ordinal and a stream, asynchronous, device pointers throughout; every argument is checked before any HIP call, a bad one
 * returns HMV_ERR_ARG with the text behind hmv_last_error(NULL) naming it, and no output is touched. */

/* Frame-space label joints into the windows a step ran on (hmv_forward_frames_track's crop_boxes BEFORE the call; SequenceTracker's
 * crop_boxes_used): batch_joints_img_to_cropped_joints (datasets/utils.py:124-143) to the bits of the reference's fp32 torch run.  Per
 * frame slot n with S = float(image_size), every operation rounded on its own (no fused multiply-add):
 *       wf = fl(float(x2) - float(x1))      d = fl(X - float(x1))      r = fl(fl(1 / wf) * S)      u = fl(d * r)      v likewise with y1, y2
 * The order matters: `image_size / widths` with a Python scalar on the left is widths.reciprocal() * image_size in torch, which differs
 * from fl(S / wf) in about a quarter of the coordinates when S is not a power of two (192, 320).
 *   joints_img     [n_slots][21][2] fp32, frame pixels;   crop_boxes [n_slots][4] int32 = x1, y1, x2, y2
 *   present        device uint8 [n_slots] or NULL (= every slot present)
 *   joints_mask_in device uint8 [n_slots][21] or NULL, non-zero = the joint is invisible (inputs["joints_img_mask"])
 *   joints_crop    [n_slots][21][2] fp32: the labels in crop pixels of the window, what inputs["joints_crop_img"] holds for a dataset box
 *   mask_out       uint8 [n_slots][21] or NULL: joints_mask_in != 0 || status != 0
 *   slot_info      int32 [n_slots][3] or NULL = { status, outside, visible }
 * status 0: mapped.
 * status 1: present[n] == 0.  joints_crop row zeros, mask_out row all 1.
 * status 2: an empty window (x2 <= x1 or y2 <= y1), which a tracker can produce (points2d_to_bbox with margin 0 on coincident
 *           joints).  The reference divides by zero there; this entry writes what status 1 writes and reports the slot, so that one
 *           such step does not poison an epoch's sums.
 * visible: the joints of a status-0 slot whose joints_mask_in is zero (21 with a NULL joints_mask_in).  outside: how many of those have a
 *          mapped coordinate that is non-finite or not in 0 <= c < S on either axis (0 is inside, S is outside).  Both 0 for status 1, 2.
 * One wave per slot, four slots per workgroup; the counts travel by ballot: no LDS, no atomics.  Outputs must not alias inputs.
 * HMV_ERR_ARG for n_slots <= 0, image_size <= 0, a NULL joints_img / crop_boxes / joints_crop. */
int hmv_op_labels_to_windows(int32_t device, int32_t n_slots, const float *joints_img, const int32_t *crop_boxes, const uint8_t *present,
                             const uint8_t *joints_mask_in, int32_t image_size, float *joints_crop, uint8_t *mask_out, int32_t *slot_info,
                             void *stream);

/* PoseMetrics.mka (models/metrics.py:36-49), the mean keypoint acceleration that measures tracking jitter; it needs no labels.
 *   preds [B][T][n_pts][dim] fp32 (dim 1 .. 4; units as given);   out [B] fp32
 * Per sequence: acc = (p[t] + p[t + 2]) - 2 p[t + 1], the norm over dim, the mean over the (T - 2) * n_pts rows; fp64 arithmetic from the
 * fp32 inputs in exactly that operation order, one rounding to fp32 at the end.  T < 3 gives NaN (the reference's mean of an empty
 * tensor).  One workgroup per sequence, fixed-order reduction: two calls give the same bits.
 * HMV_ERR_ARG for B <= 0, T < 0, n_pts <= 0, dim outside 1 .. 4, a NULL preds / out. */
int hmv_op_mka(int32_t device, const float *preds, int32_t B, int32_t T, int32_t n_pts, int32_t dim, float *out, void *stream);

/* hmv_seq_eval_add adds ONE time step of B concurrent sequences ("lanes": the tracker's batch) into caller-owned device memory, so
 * that jitter and window quality of a whole sequence are read back once.  A zero-filled pair of buffers is an empty evaluation, as
 * for hmv_eval_add; summing the `sums` of several ranks element by element (all but [0]) gives the sums of their union.
 *
 * sums: doubles [B][12] (hmv_seq_eval_sums_doubles(B)), per lane
 *   [0]   steps since the lane's last restart           [1]   steps in total
 *   [2]   acceleration rows: grows by 21 at a step once [0] >= 3
 *   [3]   sum of ||acc|| of the predictions (the units of pred_joints_cam), acc as in hmv_op_mka from this step and the two before it
 *   [4]   sum of ||acc|| of the labels; untouched when gt_joints_cam is NULL.  [4] / [2] is the labels' own jitter only for a lane that
 *         had labels at every step since its restart: a step without labels leaves the label history as it is
 *   [5 .. 7]   slot-steps with track_status 0 / 1 / 2 (window moved / view absent / window kept)
 *   [8]   slot-steps with an empty window (slot_info status 2)      [9]   sum of visible      [10]   sum of outside      [11]   0
 * history: fp32 [B][2][2][63] (hmv_seq_eval_history_floats(B)): {predictions, labels} x {step t - 2, step t - 1} x [21][3].
 * restart[b] != 0: a new sequence begins in lane b at this step.  [0] is set to 0 before the step is added, so the lane's history is
 *   not used until two further steps have filled it; the other sums keep accumulating.  The pooled jitter [3] / [2] over lanes and
 *   restarts is therefore the mean over every acceleration row of every sequence, hmv_op_mka's value for one sequence.
 * Counts are integers held in doubles.  One workgroup (one wave) per lane; a lane reads its history before it writes it and no lane
 * reads another's, so lane b of a B-lane call has the bits of a one-lane call.  The final read-modify-write of sums is by plain
 * stores from one thread per element: no floating-point atomics, fixed-order reductions.  The buffers belong to one stream at a
 * time: stream order is what orders successive steps. */
typedef struct hmv_seq_eval_args {
    int32_t struct_size;            /* sizeof(hmv_seq_eval_args), ABI guard */
    int32_t B, V;                   /* lanes, views */
    int32_t reserved;               /* 0 */
    const float *pred_joints_cam;   /* out["joints_cam"]   [B][21][3] */
    const float *gt_joints_cam;     /* labels, same shape and units; may be NULL: a live sequence has none, and jitter needs none */
    const int32_t *track_status;    /* [B][V] as hmv_forward_frames_track wrote it; may be NULL */
    const int32_t *slot_info;       /* [B][V][3] as hmv_op_labels_to_windows wrote it; may be NULL */
    const uint8_t *restart;         /* [B]; may be NULL (= no lane restarts) */
    double *sums;                   /* device, 8-byte aligned */
    float *history;                 /* device */
    size_t sums_doubles;            /* >= hmv_seq_eval_sums_doubles(B) */
    size_t history_floats;          /* >= hmv_seq_eval_history_floats(B) */
} hmv_seq_eval_args;

/* Doubles in `sums` for B lanes: 12 * B; 0 when B < 1. */
size_t hmv_seq_eval_sums_doubles(int32_t B);

/* Floats in `history` for B lanes: 252 * B; 0 when B < 1. */
size_t hmv_seq_eval_history_floats(int32_t B);

/* Adds one step, asynchronously on `stream`.  HMV_ERR_ARG for a NULL args, a wrong struct_size, B < 1, V < 1, B * V > 2^24, a NULL
 * pred_joints_cam, a NULL or misaligned sums / history, sums_doubles / history_floats below what the sizing entries give. */
int hmv_seq_eval_add(int32_t device, const hmv_seq_eval_args *args, void *stream);

/* ---- hand IK: pose parameters from 21 joints ----
 * Everything the reference's JointsToVertices.__call__ (models/joints_to_vertices.py:25-50) does around its MANO layer, per sample and
 * on the host there, as two stateless device entries (hand_ik.hip).  The MANO layer itself is the caller's (handmvnet_amd/ik.py).
 *
 * hmv_op_hand_ik: the three-point rigid alignment onto the template (rigid_transform_3D, utils/misc.py:10-47, on joints 0, 9, 13 of
 * both sides as joints_to_vertices.py:27-39 calls it) and the analytic inverse kinematics (adaptive_IK, utils/analytical_ik.py:50-138).
 *   joints           [n][21][3] fp32, the prediction in millimetres (joints_cam * 1000, handmvnet.py:396)
 *   template_joints  [21][3] fp32, the flat-hand template of the caller's MANO layer in its units; one template for every sample
 *   pose_R           [n][16][3][3] fp32: slot 0 = R[0], slot ID2ROT[k] = R_pa_k[k] (analytical_ik.py:132-136); every slot is written
 *   align            [n][12] fp64: ret_R row-major, then ret_t (fp64 because the reference keeps them in float64 for the un-alignment)
 *   joints_aligned   [n][21][3] fp32 or NULL: joints_to_mano (joints_to_vertices.py:39)
 *   status           [n] int32
 * fp64 arithmetic from the fp32 inputs in the reference's operation order, no fused multiply-add; outputs rounded once.
 *   alignment: centroids, H = Am Bm^T, R = V U^T; det(R) < 0: the last row of V^T negated and R recomputed; t = -R cA + cB.  H has rank
 *     2, the signs of the third singular vectors are arbitrary, and the determinant rule is what makes R unique: a proper rotation.
 *   global rotation: H from the five palm vectors (joints 1, 5, 9, 13, 17 minus joint 0) of the template and of the aligned joints,
 *     R0 = V U^T, then THE REFERENCE'S reflection rule, which is not the textbook one: the last column of V is negated only when
 *     |det R0 + 1| < 1e-6 AND some |S_i| < 1e-4.  A mirrored (left) hand with a non-planar palm keeps a reflection as R0.
 *   chain: the 15 joints of kinematic_tree with SNAP_PARENT as parents, the + 1e-8 terms where the reference has them, acos of the
 *     unclamped cosine, D_sw = the Rodrigues matrix of transforms3d's axangle2mat(axis, angle, is_normalized=False) (the axis divided by
 *     its norm once more; rows [xxC+c, xyC-zs, zxC+ys], [xyC+zs, yyC+c, yzC-xs], [zxC-ys, yzC+xs, zzC+c]), D_tw the same function of the
 *     template bone and angle 0, R_pa_k = D_sw D_tw, R[k] = R[pa] R_pa_k.  inv(R[pa]) is the transpose: R[pa] is R0 times Rodrigues
 *     matrices, orthogonal by construction, a reflection R0 included.
 * status 0: the normal case.
 * status 1: some written value (pose_R, align, joints_aligned whether or not it is requested) is non-finite: a non-finite input, a
 *           target bone exactly collinear with its template bone, coincident points, a cosine above 1, a zero template bone.  The
 *           reference produces NaN there too; the values are written as computed, nothing is repaired.
 * One wave64 per sample, four samples per workgroup; the two SVDs on one lane, the five fingers on five; no LDS, no atomics.  Row i of
 * an n-row call has the bits of a one-row call.  Outputs must not alias inputs.  Takes no handle; asynchronous on `stream`.
 * HMV_ERR_ARG before any HIP call (hmv_last_error(NULL) names the argument) for n <= 0, a NULL joints / template_joints / pose_R /
 * status, a NULL or misaligned align. */
int hmv_op_hand_ik(int32_t device, const float *joints, const float *template_joints, int32_t n, float *pose_R, double *align,
                   float *joints_aligned, int32_t *status, void *stream);

/* The inverse of that alignment on any points (joints_to_vertices.py:48: the MANO vertices back to where the joints were):
 *   out[i][p] = R_i^T (points[i][p] - t_i)   with (R_i, t_i) = align[i], in fp64, rounded once to fp32
 *   points, out  [n][n_pts][3] fp32, may be the same buffer;   align [n][12] fp64 as hmv_op_hand_ik wrote it
 * HMV_ERR_ARG before any HIP call for n <= 0, n_pts <= 0, a NULL points / out, a NULL or misaligned align. */
int hmv_op_rigid_unapply(int32_t device, const float *points, const double *align, int32_t n, int32_t n_pts, float *out, void *stream);

/* ---- MANO skinning: 16 rotation matrices and 10 shape coefficients to the mesh and the 21 joints ----
 * The published MANO / SMPL blend-skinning formula in the order ManoLayer.forward applies it with root_rot_mode = joint_rot_mode =
 * "rotmat", use_pca=False and no th_trans / center_idx (the reference's configuration, models/joints_to_vertices.py:14-20), as one
 * stateless launch over a packed parameter buffer (mano_skin.hip).  manopth and the MANO files are not part of this repository: the
 * arithmetic is pinned to the formula below (tests/mano_oracle.py repeats it in float64), not to the package's bits.
 *
 * Parameters, fp32 DEVICE arrays in MANO's own layouts, Nv = n_verts:
 *   v_template [Nv][3]   shapedirs [Nv][3][10]   posedirs [Nv][3][135]   J_regressor [16][Nv]   weights [Nv][16]
 *   tips [5] (HOST values in the struct): the vertex indices of the thumb, index, middle, ring and little finger tips
 *   parents of joints 0..15: -1,0,1,2,0,4,5,0,7,8,0,10,11,0,13,14
 * hmv_op_mano_pack writes them once into `packed`, hmv_mano_pack_bytes(n_verts) bytes (0 for n_verts outside 1 .. 2^20), 8-byte
 * aligned: 528 doubles (J_regressor . v_template [16][3], then J_regressor . shapedirs [16][3][10], each a sum over the vertices in
 * ascending order in fp64), 8 int32 (tips, n_verts, 0, 0), then 454 planes of Nv floats: v_template [3][Nv], shapedirs [10][3][Nv],
 * posedirs [135][3][Nv], weights [16][Nv].  No skin launch touches the regressor or the MANO layouts.
 *
 * hmv_op_mano_skin, per row, in fp64 from the fp32 inputs, no fused multiply-add, every output rounded once:
 *   1. project != 0: each of the 16 matrices becomes Q = U V^T of its SVD, column 2 of Q negated when det Q < 0 (the polar factor,
 *      made a rotation: what manopth's rotproj does in rotmat mode; it turns the reflection hmv_op_hand_ik keeps as slot 0 for a
 *      mirrored hand into a rotation).  project == 0: the matrices are used as given.
 *   2. v_shaped = v_template + shapedirs . betas;   J = J_regressor . v_shaped  (from the folded sums of the packed buffer)
 *   3. v_posed = v_shaped + posedirs . vec(rot[1..15] - I), the 135 values in slot order, row-major
 *   4. G[0] = [rot[0] | J[0]],  G[k] = G[parent k] . [rot[k] | J[k] - J[parent k]]
 *   5. A[k] = G[k] with its translation reduced by G[k].R . J[k]
 *   6. vertex v = (sum_k weights[v][k] A[k]) . [v_posed[v]; 1]
 *   7. joints: the 16 translations of G, then the five tip vertices, reordered by [0,13,14,15,16,1,2,3,17,4,5,6,18,10,11,12,19,7,8,9,20]
 *   8. everything times 1000 (metres to millimetres);  with `align` ([n][12] fp64 as hmv_op_hand_ik wrote it), then R^T (x - t): the mesh
 *      back where the prediction was, in the same pass
 *   rot       [n][16][3][3] fp32, slot 0 the global rotation
 *   betas     NULL with HMV_MANO_BETAS_NONE (zeros), [10] with HMV_MANO_BETAS_SHARED, [n][10] with HMV_MANO_BETAS_PER_ROW
 *   vertices  [n][Nv][3] fp32 or NULL;   joints [n][21][3] fp32 or NULL; not both NULL.  A call without vertices gives the joints the
 *             bits they have in a call with them.
 *   status    [n] int32: 1 when some value of the row (vertices when requested, joints whether or not requested) is non-finite.  The
 *             values are written as computed; a bad row marks itself alone.
 * A `packed` that was written for another n_verts is seen on the device: every value of the call is NaN, every status 1.
 * One workgroup of 512 threads per row (the status is an OR over the row and there are no atomics, so a row has one owner); row i of
 * an n-row call has the bits of a one-row call.  Outputs must not alias inputs.  Both entries take no handle and are asynchronous on
 * `stream`.
 * HMV_ERR_ARG before any HIP call (hmv_last_error(NULL) names the argument) for: a NULL params / args, another struct_size, n <= 0,
 * n_verts outside 1 .. 2^20, a NULL parameter array, a tip outside [0, n_verts), a NULL or misaligned packed, a NULL rot / status, an
 * unknown betas_mode, a betas_mode other than NONE with a NULL betas, a misaligned align, vertices and joints both NULL. */
enum { HMV_MANO_BETAS_NONE = 0, HMV_MANO_BETAS_SHARED = 1, HMV_MANO_BETAS_PER_ROW = 2 };

typedef struct hmv_mano_params {
    int32_t struct_size;   /* sizeof(hmv_mano_params) */
    int32_t n_verts;
    int32_t tips[5];
    int32_t reserved;      /* 0 */
    const float *v_template;
    const float *shapedirs;
    const float *posedirs;
    const float *J_regressor;
    const float *weights;
} hmv_mano_params;

typedef struct hmv_mano_skin_args {
    int32_t struct_size;   /* sizeof(hmv_mano_skin_args) */
    int32_t n;
    int32_t n_verts;
    int32_t betas_mode;    /* HMV_MANO_BETAS_* */
    int32_t project;
    int32_t reserved;      /* 0 */
    const void *packed;
    const float *rot;
    const float *betas;
    const double *align;   /* or NULL */
    float *vertices;
    float *joints;
    int32_t *status;
} hmv_mano_skin_args;

size_t hmv_mano_pack_bytes(int32_t n_verts);
int hmv_op_mano_pack(int32_t device, const hmv_mano_params *params, void *packed, void *stream);
int hmv_op_mano_skin(int32_t device, const hmv_mano_skin_args *args, void *stream);

/* ---- pose consensus: the S estimates of a reference-view sweep in one camera's frame, their consensus and their disagreement ----
 * Every camera of a rig can serve as reference view (hmv_forward_orders), which gives S root-relative estimates of the same hand, estimate
 * s in the frame of camera ref_cam[s].  One stateless launch (pose_consensus.hip) rotates them into camera target_cam's frame by the
 * extrinsics and reduces them per joint.
 *   poses      [S][B][21][3] fp32, root-relative (hmv_forward_orders' joints_cam)
 *   ref_cam    DEVICE int32 [S]: the camera whose frame estimate s is in
 *   extrinsic  [B][V][4][4] fp32, the reference's convention: world = E [x; 1] (utils/camera.py:4-22)
 *   mode       0 = mean, 1 = geometric median (Weiszfeld);   iterations: Weiszfeld steps (the Python layer passes 16), unused by mode 0
 *   aligned    [S][B][21][3]  estimate s in target_cam's frame
 *   consensus  [B][21][3]
 *   spread     [B][21]   sqrt(sum_s |aligned_s - consensus|^2 / S) per joint, in the poses' unit (metres)
 *   deviation  [S][B]    the mean over the 21 joints of |aligned_s - consensus|
 * Each output may be NULL, not all four.  Outputs must not alias inputs.
 * fp64 arithmetic from the fp32 inputs, no fused multiply-add, in this order (tests/consensus_oracle.py repeats it); outputs rounded once:
 *   T = rows 0..2 of inverse(E[b][target_cam]): cofactors over 2x2 minors divided by the determinant (the routine of hmv_project_joints)
 *   M[r][c] = ((T[r][0] E[0][c] + T[r][1] E[1][c]) + T[r][2] E[2][c]) + T[r][3] E[3][c]  with E = E[b][ref_cam[s]], c < 3
 *   aligned[r] = (M[r][0] x[0] + M[r][1] x[1]) + M[r][2] x[2]: the poses are root-relative, so no translation applies -- this is
 *     transform_joints_between_cameras(x) - transform_joints_between_cameras(0)
 *   mean: the sum over s ascending from 0.0, divided by S
 *   median, per joint: y_0 = the mean; y_{k+1} = (sum_s x_s / m_s) / (sum_s 1 / m_s) with m_s = max(|x_s - y_k|, 1e-12), both sums over
 *     s ascending from 0.0; exactly `iterations` steps, no early exit.  |v| = sqrt((v0 v0 + v1 v1) + v2 v2) everywhere
 *   deviation: the 21 distances summed in joint order from 0.0, divided by 21
 * A singular E[b][target_cam] gives non-finite outputs for sample b, as in hmv_project_joints.  ref_cam is device data and cannot be
 * refused: a value outside [0, V) is clamped for the load and makes that estimate's aligned row and deviation NaN -- and through them the
 * consensus and the spread.
 * One wave64 per sample, four samples per workgroup, lanes 0..20 one joint each; no LDS, no atomics.  Row b of a B-row call has the bits
 * of a one-row call.  Takes no handle; asynchronous on `stream`.
 * HMV_ERR_ARG before any HIP call (hmv_last_error(NULL) names the argument) for: a NULL args, a struct_size other than
 * sizeof(hmv_consensus_args), S, B or V below 1, target_cam outside [0, V), a mode other than 0 or 1, iterations < 0, a NULL poses /
 * ref_cam / extrinsic, all four outputs NULL. */
typedef struct hmv_consensus_args {
    int32_t struct_size;   /* sizeof(hmv_consensus_args) */
    int32_t S, B, V;
    int32_t target_cam;
    int32_t mode;
    int32_t iterations;
    int32_t reserved;      /* 0 */
    const float *poses;
    const int32_t *ref_cam;
    const float *extrinsic;
    float *aligned;
    float *consensus;
    float *spread;
    float *deviation;
} hmv_consensus_args;

int hmv_op_pose_consensus(int32_t device, const hmv_consensus_args *args, void *stream);

/* ---- triangulation: the per-view 2D joints to one 3D point per joint, DLT or DLT + RANSAC over a caller-ordered candidate table ----
 * The reference's utils/triangulation.py (batch_triangulate_dlt_torch :99-139, batch_triangulate_dlt_ransac_torch :5-58,
 * calculate_reprojection_error :61-95) as one stateless launch (triangulate.hip), with two deliberate differences: the homogeneous
 * coordinate is divided out WITHOUT the + 1e-7 of :137 (as triangulate_dlt_torch :170 and triangulate_one_point_dlt :201 do), and the
 * candidates come as an ORDERED TABLE from the caller instead of random.shuffle on the process-global state (:26).
 *   points      [B][V][J][2] fp32, 1 <= J <= 64: frame pixels; with `bbox`, crop pixels that are first mapped to the frame
 *   bbox        NULL, or [B][V][4] fp32 (x1, y1, x2, y2): X = u * ((x2 - x1) / image_size) + x1, Y likewise, in fp32, every operation
 *               rounded on its own -- batch_cropped_joints_to_joints_img (datasets/utils.py:146-162) in the operation order of
 *               hmv_op_next_crop_boxes, whose joints_img has the same bits
 *   intrinsic   [B][V][4] fp32 (fx, fy, cx, cy)
 *   extrinsic   [B][V][4][4] fp32.  extrinsic_kind 0: camera-to-world, world = E [x; 1] (the data set's cam_params["extrinsic"],
 *               utils/camera.py:17-20) -- inverted here by the cofactor routine of hmv_project_joints;  1: world-to-camera, what
 *               triangulation.py takes
 *   present     NULL, or [B][V] uint8, zero = the view is absent
 *   joint_mask  NULL, or [B][V][J] uint8, NON-zero = do not use this view for this joint (the sense of joints_img_mask)
 *               A view is USABLE for joint j when it is present and not masked.
 *   subsets     NULL (one DLT over all usable views), or DEVICE int32 [S][n_cams]: candidate s names n_cams cameras
 *   threshold   pixels, read with a table only;  refit: 0 or 1, read with a table only
 *   frame_cam   NULL (world coordinates), or DEVICE int32 [B]: the result in that camera's frame, W [X; 1] with W the world-to-camera
 *               rows of that camera (inverse(E) for kind 0)
 *   points3d    [B][J][3] fp32
 *   reproj_err  NULL, or [B][V][J] fp32: the written point's reprojection error in every view, NaN for a view that is not usable
 *   inliers     NULL, or [B][J] int32: the winner's inlier count; without a table the number of usable views
 *   winner      NULL, or [B][J] int32: the winner's index into `subsets`; -1 without a table and for status 1 and 2
 *   status      [B][J] int32
 * The rule, in fp64 from the fp32 inputs, no fused multiply-add, outputs rounded once:
 *   W_v = rows 0..2 of the world-to-camera matrix;  M_v[r][c] = K_v W_v: rows (fx W0 + cx W2), (fy W1 + cy W2), W2
 *   the DLT rows of view v: x M_v[2] - M_v[0], then y M_v[2] - M_v[1] (:128-134);  X = v[:3] / v[3] with v the right singular vector of
 *   the smallest singular value: the rows are rotated one by one (Givens) into a 4x4 triangular factor, whose singular vectors a
 *   one-sided Jacobi iteration of a fixed number of sweeps finds -- no normal equations
 *   no table: one DLT over the usable views, ascending
 *   a table:  candidate s is the DLT over its cameras in the order the row lists them; a candidate that names a camera outside [0, V) or
 *             one that is not usable is SKIPPED; its inlier count is the number of usable views with |proj - point| < threshold,
 *             proj = (M [X; 1])[:2] / (M [X; 1])[2], the error sqrt(dx dx + dy dy); the FIRST candidate with the most inliers wins
 *   refit 1:  the output is the DLT over the winner's inlier views, ascending, when there are at least two of them (not in the reference)
 * status: 0 ok;  1 no candidate had an inlier: the point is 0, 0, 0 as the reference leaves it;  2 fewer than two usable views, or every
 * candidate was skipped: the point is NaN;  3 a written coordinate is not finite (a singular extrinsic, coincident cameras, a NaN input,
 * a frame_cam outside [0, V)).  Device code reports, it does not repair.
 * One wave64 per (sample, joint), four per workgroup; the V projection matrices sit in LDS, lanes stride over the candidates; no
 * atomics.  The bits of (b, j) depend on neither B nor the row's place in the call; a masked call has the bits of the call on the
 * reduced camera list.  Takes no handle; asynchronous on `stream`.  Outputs must not alias inputs.
 * HMV_ERR_ARG before any HIP call (hmv_last_error(NULL) names the field) for: a NULL args, a struct_size other than
 * sizeof(hmv_triangulate_args), B < 1 or B * J beyond 2^24, V outside [1, 16], J outside [1, 64], a NULL points / intrinsic / extrinsic /
 * points3d / status, a table with S outside [1, 4096] or n_cams outside [2, V], a threshold that is not finite or <= 0 with a table, a bbox
 * with image_size < 1, an extrinsic_kind or a refit other than 0 or 1. */
typedef struct hmv_triangulate_args {
    int32_t struct_size;   /* sizeof(hmv_triangulate_args) */
    int32_t B, V, J;
    int32_t S, n_cams;     /* the table's shape; ignored when subsets is NULL */
    int32_t image_size;    /* read with bbox */
    int32_t extrinsic_kind;
    int32_t refit;
    float threshold;
    const float *points;
    const float *bbox;
    const float *intrinsic;
    const float *extrinsic;
    const uint8_t *present;
    const uint8_t *joint_mask;
    const int32_t *subsets;
    const int32_t *frame_cam;
    float *points3d;
    float *reproj_err;
    int32_t *inliers;
    int32_t *winner;
    int32_t *status;
} hmv_triangulate_args;

int hmv_op_triangulate(int32_t device, const hmv_triangulate_args *args, void *stream);

/* ---- heat-map confidences: the peak of every score map, and the views a confidence threshold keeps per joint ----
 * Two stateless launches (confidence.hip) that put the reference's confidence-gated triangulation on the device:
 * heatmaps_to_coordinates (models/utils.py:65-82) and the camera selection of triangulate_dlt (utils/triangulation.py:227-236).
 * The selection's mask_out is hmv_op_triangulate's joint_mask; the triangulation itself is that entry, unchanged.
 *
 * hmv_op_heatmap_peaks
 *   heatmap   [N][J][h][w] fp32, contiguous: the NCHW map every forward returns (N = frames)
 *   maxval    NULL, or [N][J] fp32: the maximum of the map
 *   index     NULL, or [N][J] int32: where it lies, flat y * w + x, 0-based
 *   preds     NULL, or [N][J][2] fp32: the reference's 1-based (index % w + 1, index / w + 1), times (maxval > 0)
 *   (not all three NULL)
 * The rule is torch.max(scores.view(N, J, -1), 2): the largest value wins; among equal values the LOWEST flat index wins (+0 and -0 are
 * equal); a NaN beats every number and the FIRST NaN wins -- the NaN in maxval is the report, its preds are 0; a map of -inf only gives
 * -inf at index 0.  One wave64 per map, four per workgroup; 16-byte loads when h * w is a multiple of 4 and heatmap is 16-byte aligned,
 * scalar loads otherwise: the same bits either way.  The bits of a map depend on neither N nor its place in the call.  No byte outside
 * the maps is read.
 * HMV_ERR_ARG before any HIP call for: a NULL args, a struct_size other than sizeof(hmv_peaks_args), N, J, h or w below 1, N * J beyond
 * 2^24, h * w beyond 2^20, a NULL heatmap, all three outputs NULL.
 *
 * hmv_op_confidence_select
 *   conf        [B][V][J] fp32: maxval of a [B * V] frame batch as it lies
 *   present     NULL, or [B][V] uint8;  joint_mask  NULL, or [B][V][J] uint8: the senses of hmv_op_triangulate
 *   threshold, step   doubles;  carry  0 or 1
 *   mask_out    [B][V][J] uint8: 1 = leave this view out for this joint.  It includes the caller's joint_mask and absent views: feed it
 *               to hmv_op_triangulate as joint_mask
 *   level       NULL, or [B][J] fp32: the threshold that decided, (float)t
 *   lowered     NULL, or [B][J] int32: the decrements spent on this joint
 *   selected    NULL, or [B][J] int32: the views kept
 * The rule, per sample (t is a double, lowered by repeated subtraction, never recomputed from a level count):
 *   t = threshold                       -- once per sample when carry == 1: what joint j lowered, every later joint starts from, as in the
 *                                          reference, which never resets it;  for every joint anew when carry == 0
 *   for j:  loop { sel_v = usable(v, j) && conf[v][j] > (float)t;  n = count(sel)
 *                  if (t <= 0) break;  if (n <= 1) { t -= step; ++lowered[j]; } else break; }
 *           mask_out[v][j] = !sel_v;  level[j] = (float)t;  selected[j] = n
 * The comparison is made in fp32 with t rounded to fp32 -- what numpy makes of float32_array > python_float -- so float32(0.4) > 0.4 is
 * false.  A view that is not usable is neither selected nor counted: a gated call has the decisions of the call on the reduced camera
 * list.  A NaN confidence is never selected.  Deliberately different from the reference in one way: where t reaches <= 0 with fewer than
 * two views selected the reference triangulates from one camera or raises; here `selected` says so and hmv_op_triangulate reports status
 * 2 and NaN for that joint.  One wave64 per sample, four per workgroup; at most threshold / step + 2 ballots per level walk.
 * HMV_ERR_ARG before any HIP call for: a NULL args, a struct_size other than sizeof(hmv_confidence_select_args), B < 1, V outside
 * [1, 16], J outside [1, 64], a carry other than 0 or 1, a threshold or a step that is not finite, step <= 0, threshold / step > 1024,
 * a NULL conf or mask_out.
 * Both take no handle, are asynchronous on `stream`, use no atomics; outputs must not alias inputs. */
typedef struct hmv_peaks_args {
    int32_t struct_size;   /* sizeof(hmv_peaks_args) */
    int32_t N, J, h, w;
    const float *heatmap;
    float *maxval;
    int32_t *index;
    float *preds;
} hmv_peaks_args;

int hmv_op_heatmap_peaks(int32_t device, const hmv_peaks_args *args, void *stream);

typedef struct hmv_confidence_select_args {
    int32_t struct_size;   /* sizeof(hmv_confidence_select_args) */
    int32_t B, V, J;
    int32_t carry;
    double threshold, step;
    const float *conf;
    const uint8_t *present;
    const uint8_t *joint_mask;
    uint8_t *mask_out;
    float *level;
    int32_t *lowered;
    int32_t *selected;
} hmv_confidence_select_args;

int hmv_op_confidence_select(int32_t device, const hmv_confidence_select_args *args, void *stream);

/* ---- windows from the reprojected pose: the crop windows of ALL cameras of a sample from one 3D pose ----
 * hmv_op_next_crop_boxes moves a camera's window to the box around that camera's own 2D joints: a view that loses the hand loses its
 * window, and an absent view returns to a stale one.  This launch (track.hip) moves the windows of every camera to where ONE 3D pose --
 * the triangulated joints, or the model's joints_cam on the triangulated root -- projects: get_2d_joints_from_3d_joints
 * (utils/camera.py:25-44, the arithmetic of hmv_project_joints) followed by points2d_to_bbox (datasets/utils.py:5-27, the integer rule
 * of hmv_op_next_crop_boxes), per slot (b, v).  It runs BEHIND the own-joints rule, in place on its windows and status, which stay
 * wherever this launch does not move them.
 *   points3d      [B][21][3] fp32, metres, in the frame of camera frame_cam[b]
 *   point_status  NULL, or [B][21] int32: hmv_op_triangulate's status of every joint
 *   frame_cam     NULL (camera 0), or DEVICE int32 [B]
 *   intrinsic     [B][V][4] fp32 (fx, fy, cx, cy);  extrinsic [B][V][4][4] fp32, camera-to-world as hmv_project_joints takes them
 *   joints_img    NULL, or [B][V][21][2] fp32: the views' own 2D joints in frame pixels, read for `gap` only
 *   crop_boxes    [B][V][4] int32, in / out;  bbox NULL, or [B][V][4] fp32, in / out: the same four numbers as fp32
 *   status        [B][V] int32, in / out: hmv_op_next_crop_boxes' 0 moved / 1 absent / 2 kept
 *   source        [B][V] int32, out: 0 = the window is the own-joints rule's (or whatever crop_boxes held), 1 = it is the reprojection's
 *   joints_reproj NULL, or [B][V][21][2] fp32, out: the projections in frame pixels
 *   gap           NULL, or [B][V] fp32, out
 * A sample is OK when its 63 coordinates are finite, frame_cam[b] lies in [0, V) and point_status is NULL or point_status[b][0] == 0
 * (the root was triangulated) -- with require_all != 0: all 21 entries are 0.
 * Slot (b, v) of an OK sample is REPROJECTED when every one of its 21 joints has a positive depth term z = z_cam * 1000 + 1e-6 (the
 * reference's unit and epsilon), finite u and v of magnitude below 1e9, and the window of the 21 projections is at most 65536 px wide
 * and tall.  Such a slot: crop_boxes = points2d_to_bbox(projections, margin, square), bbox its fp32, source 1; status 2 becomes 0, 0 stays
 * 0, 1 stays 1 (the window moves, the view is still absent: the three window fractions of hmv_seq_eval_add still sum to one).
 * Any other slot: source 0; not one byte of its crop_boxes, bbox and status is written.
 * joints_reproj is the projection in fp64 from the fp32 inputs, rounded once -- the bits of hmv_project_joints without bbox -- written as
 * computed for every slot of an OK sample, NaN for a sample that is not.
 * gap[b][v] = the mean over the 21 joints of |joints_img - joints_reproj|, in fp64 from the fp32 values as written, rounded once: how far
 * this camera's own joints are from what the others agree on, in frame pixels.  Defined when joints_img is given, the sample is OK and
 * the INCOMING status is 0; NaN otherwise.  An output only: no rule reads it.
 * One wave64 per slot, four per workgroup, a joint per lane; minimum, maximum and the gap's sum by fixed-order shuffles; no LDS, no
 * atomics.  The bits of a slot depend on neither B nor its place in the call.  Takes no handle; asynchronous on `stream`.
 * HMV_ERR_ARG before any HIP call, the outputs untouched, for: a NULL args, a struct_size below sizeof(hmv_reproject_boxes_args), B < 1,
 * B * V beyond 2^24, V outside [1, 16] (hmv_op_triangulate's), margin < 0, a NULL points3d / intrinsic / extrinsic / crop_boxes /
 * status / source. */
typedef struct hmv_reproject_boxes_args {
    int32_t struct_size;   /* sizeof(hmv_reproject_boxes_args) */
    int32_t B, V;
    int32_t margin;
    int32_t square;
    int32_t require_all;
    const float *points3d;
    const int32_t *point_status;
    const int32_t *frame_cam;
    const float *intrinsic;
    const float *extrinsic;
    const float *joints_img;
    int32_t *crop_boxes;
    float *bbox;
    int32_t *status;
    int32_t *source;
    float *joints_reproj;
    float *gap;
} hmv_reproject_boxes_args;

int hmv_op_reproject_crop_boxes(int32_t device, const hmv_reproject_boxes_args *args, void *stream);

const char *hmv_version(void);

/* The tile shape the general conv / GEMM kernel's launcher rule picks for M output pixels, Cout channels, reduction length K
 * (e.g. "256x256", "128x32", "256x128,k16,w8"); host logic only, valid until the calling thread's next call. */
const char *hmv_tile_rule(int32_t M, int32_t Cout, int32_t K, int32_t f16, int32_t has_residual);

#ifdef __cplusplus
}
#endif
#endif /* HANDMV_H */
