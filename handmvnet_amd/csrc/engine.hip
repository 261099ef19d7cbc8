// engine.hip -- host side of libhandmv.so: weight ingestion (BN folding, K-major repack),
// workspace planning and the forward orchestration behind the C ABI of include/handmv.h.
//
// The forward mirrors HandMvNet.forward (/root/reference/src/models/handmvnet.py:158-266)
// stage by stage, but NHWC end to end and with every conv/linear routed to the one
// implicit-GEMM MFMA kernel family (conv_igemm.hip).  There is no CPU fallback: every
// entry point needs a HIP device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/handmv.h"
#include "kernels.h"

using namespace hmv;

namespace {

constexpr int NJ = 21, HEADS = 8, DHEAD = 128, INNER = HEADS * DHEAD;
constexpr int DHEAD_LQ = 256, INNER_LQ = HEADS * DHEAD_LQ;   // MultiHeadAttentionLearnableQuery, layers.py:241
const int kBlocks[3][4] = {{2, 2, 2, 2}, {3, 4, 6, 3}, {3, 4, 6, 3}};
const int kHrChannels[2][4] = {{40, 80, 160, 320}, {64, 128, 256, 512}};   // hrnet.py:430-447
inline int cpad(int c) { return (c + 3) / 4 * 4; }   // NHWC channel stride: 16-byte pixels are all the conv kernel needs

thread_local std::string g_create_err;   // hmv_last_error(NULL): per thread, like errno

// The range word of ONE op-level call (hmv_op_* entries in the (hi, lo) pair modes): the call's pair conversions report a clamped value
// into it (note_range, kernels.h) and the entry returns HMV_ERR_RANGE after synchronising.
struct RangeWord {
    int *p = nullptr;
    hipError_t alloc() {
        const int zero = 0;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), sizeof(int));
        if (e == hipSuccess) e = hipMemcpy(p, &zero, sizeof(int), hipMemcpyHostToDevice);
        return e;
    }
    bool saturated() const {   // after the call's stream has been synchronised
        int v = 0;
        return p && hipMemcpy(&v, p, sizeof(int), hipMemcpyDeviceToHost) == hipSuccess && v != 0;
    }
    ~RangeWord() { if (p) (void)hipFree(p); }
};
const char *const kRangeMsg = "a value outside the (hi, lo) fp16 pair range (|v| > 65504) was clamped: the result is not fp32-equivalent";

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
};

// One GEMM-shaped layer on the device: Wt [Cout_pad][Kpad] + bias [Cout_pad].
struct Layer {
    float *w = nullptr, *bias = nullptr;
    int Cin = 0, Cout = 0, R = 1, S = 1, K = 0, Kpad = 0, Cout_pad = 0;
    int Kreal = 0;      // reduction length without channel padding (FLOP accounting)
    int in_real = 0;    // real input elements per input pixel when that is not Kreal / (R * S) (the space-to-depth stem)
    int acc_shift = 0;  // HMV_F32X3: the packed weights are W * 2^acc_shift, the epilogue scales the accumulator back
    bool x3n = false;   // HMV_F32X3: fused split reduction (one tile load per three products; conv_igemm.hip), else the cwrap scheme
    int plane = 0;      // HMV_F32X3 (split operands): physical channels per (hi | lo) plane; Cin is then the virtual 3 * plane
    int rd_cout = 0;    // row-decomposed 3x3 (conv_igemm.hip, RD): the real Cout; Cout / R / S then describe the 3x1 GEMM
    bool f16 = false;   // operands (activations + packed weights) are fp16; bias stays fp32
    bool tall = false;  // fp16 3x3 packed in conv_ht.hip's K order (32-channel chunk, r, s, c % 32): runs on that kernel at every batch
    std::string label;
};

struct Block {
    Layer c1, c2, c3, ds;
    bool has_ds = false;
    int stride = 1;
    // Bottleneck with a downsample branch: conv3 + BN3 and downsample conv + BN as ONE GEMM over the concatenated reduction
    // [t2 | x] . [s3 W3 ; sds Wds] + (b3 + bds) -- the downsample output is never written or re-read (resnet.py:124-144)
    Layer c3ds;
    bool fused_ds = false;
};

// HRNet (backbones/hrnet.py): one HighResolutionModule = per-branch BasicBlocks + the fuse layers
struct HrModule {
    Layer br[4][4][2];             // [branch][block][conv1 | conv2]
    std::vector<Layer> fuse[4][4]; // [i][j]: j > i one 1x1 conv; j < i a chain of (i - j) stride-2 3x3 convs
    Layer fup[4][4];               // fp16 mode: the j > i 1x1 convs once more as fp32 [Cout][Cin] for hr_fuse.hip (the fp32 mode reads fuse[i][j][0])
};
struct HrNet {
    Layer conv1, conv2;            // stem: two 3x3 stride-2 convs
    std::vector<Block> layer1;     // 4 Bottlenecks (planes 64)
    std::vector<Layer> trans[3][4];
    std::vector<HrModule> stage[3];
    int ch[4] = {0, 0, 0, 0};
};

struct AttnLayer {
    Layer qkv, out, ff1, ff2;
    Layer out_x3;   // fp16-kernel modes: to_out once more as a split-pair GEMM (Loader::linear_x3; gemm_x3.hip), fed by attention rows
                    // written as (hi, lo) pairs; its bias stays with `out` (ff_block_kernel adds it)
    float *n1g = nullptr, *n1b = nullptr, *n2g = nullptr, *n2b = nullptr, *fg = nullptr, *fb = nullptr;
    // learnable-query fusion (layers.py:240-301): the probe block projects only K and V from the tokens; its queries
    // to_q(probe + PE) do not depend on the input and are computed once at load time ([21][2048])
    Layer kv;
    float *qprobe = nullptr;
};

// First-fit planner over one contiguous arena.  Run once "dry" to size the workspace and
// once for real; both runs issue the same alloc/free sequence so offsets agree.
struct Arena {
    struct Seg { size_t off, size; };
    std::vector<Seg> free_list;  // sorted by offset
    std::map<size_t, size_t> live;
    size_t high = 0, top = 0;
    char *base = nullptr;
    void reset(char *b) { free_list.clear(); live.clear(); high = top = 0; base = b; }
    float *alloc(size_t floats) {
        size_t bytes = (floats * sizeof(float) + 255) / 256 * 256;
        if (bytes == 0) bytes = 256;
        for (size_t i = 0; i < free_list.size(); ++i) {
            if (free_list[i].size >= bytes) {
                size_t off = free_list[i].off;
                if (free_list[i].size == bytes) free_list.erase(free_list.begin() + i);
                else { free_list[i].off += bytes; free_list[i].size -= bytes; }
                live[off] = bytes;
                return reinterpret_cast<float *>(base + off);
            }
        }
        size_t off = top;
        top += bytes;
        if (top > high) high = top;
        live[off] = bytes;
        return reinterpret_cast<float *>(base + off);
    }
    void release(float *p) {
        if (!p) return;
        size_t off = (size_t)(reinterpret_cast<char *>(p) - base);
        auto it = live.find(off);
        if (it == live.end()) return;
        Seg s{off, it->second};
        live.erase(it);
        size_t i = 0;
        while (i < free_list.size() && free_list[i].off < s.off) ++i;
        free_list.insert(free_list.begin() + i, s);
        // coalesce neighbours
        if (i + 1 < free_list.size() && free_list[i].off + free_list[i].size == free_list[i + 1].off) {
            free_list[i].size += free_list[i + 1].size;
            free_list.erase(free_list.begin() + i + 1);
        }
        if (i > 0 && free_list[i - 1].off + free_list[i - 1].size == free_list[i].off) {
            free_list[i - 1].size += free_list[i].size;
            free_list.erase(free_list.begin() + i);
            --i;
        }
        if (!free_list.empty() && free_list.back().off + free_list.back().size == top) {
            top = free_list.back().off;
            free_list.pop_back();
        }
    }
};

struct ProfRec {
    const char *name;
    std::string label;
    double flops;
    double bytes;   // algorithmic HBM bytes of the launch: every operand / result element moved once
    hipEvent_t e0, e1;
};

}  // namespace

struct hmv_engine {
    hmv_config cfg{};
    std::string err;
    std::map<std::string, HostTensor> host;
    bool finalized = false;
    std::vector<void *> dev_allocs;

    // derived shape facts
    int d = 0, ldt = 0, fdim = 0;
    bool paper = false;
    bool lq = false;   // model.fusion == cross_attn_learnable_query

    Layer stem;
    HrNet hr;
    bool hrnet = false;
    std::vector<Block> blocks[3];
    Layer pose0, pose1, pose2;   // r50: pose0 (1x1 1024->512), pose1 (1x1 512->21); r18/34: pose1 (3x3 128->64), pose2 (3x3 64->21)
    Layer deconv[4];             // r18/34 ConvTranspose2d as 4 sub-pixel 2x2 convs (phase a*2+b)
    Layer deconv_all;            // ... the same four with their weight blocks back to back (one launch); w == nullptr: not used
    size_t deconv_stride = 0;    // elements between the phases' weight blocks
    Layer sample[4];
    std::vector<AttnLayer> attn;
    Layer gcn[3];
    float *gcn_bias[3] = {nullptr, nullptr, nullptr};
    float *cheb_t = nullptr;
    Layer fc1, fc2;
    float *pe = nullptr;
    float *zero_bias = nullptr;   // 4096 zeros: bias of split-K slices

    char *arena = nullptr;
    size_t arena_bytes = 0;
    int reserved_batch = 0;
    Arena plan;

    // ragged view sets (hmv_forward_views): the call's tables [seg: B + 1 first token rows | fpos: per frame, 21 x its rank among its
    // sample's present views] -- the host copy, and the device copy it is uploaded to on the caller's stream.  The host copies are
    // pinned (the upload is then asynchronous for the host as well) and form a small ring: a slot is rewritten only after the upload
    // that last read it has run (`done`), which a caller notices only when it is four ragged calls ahead of the device.
    struct ViewsSlot { int32_t *host = nullptr; size_t cap = 0; hipEvent_t done = nullptr; };
    ViewsSlot views_host[4];
    unsigned views_next = 0;
    int32_t *views_dev = nullptr;
    size_t views_cap = 0;
    bool last_ragged = false;   // the last forward was a ragged one: it captured no stages (hmv_read_stage)

    bool capture = false;
    int cap_batch = 0;
    float *cap_feat0 = nullptr, *cap_coords = nullptr, *cap_tokens = nullptr, *cap_fused = nullptr;
    size_t cap_feat0_n = 0, cap_coords_n = 0, cap_tokens_n = 0, cap_fused_n = 0;

    // attention maps (hmv_set_attention_capture; attention_probs.hip): bit l of att_mask selects fusion block l.  A selected block owns a map
    // and a view-share buffer outside the workspace, sized for att_batch full-view samples (ensure_attention); B / Tq / Tk / views are
    // what the LAST forward left in them (valid: it did; every forward and sweep clears it first).  A non-zero mask keeps forwards eager.
    struct AttMap {
        float *probs = nullptr, *share = nullptr;
        size_t probs_cap = 0, share_cap = 0;
        bool valid = false;
        int B = 0, Tq = 0, Tk = 0, views = 0;
    };
    uint32_t att_mask = 0, att_alloc_mask = 0;   // selected now / what the buffers were allocated for
    int att_batch = 0;
    std::vector<AttMap> att;
    int fusion_blocks() const { return lq ? 5 : cfg.fusion_layers; }
    int cross_block() const { return lq ? 2 : (cfg.fusion_layers - 1) / 2; }
    void forget_attention() {
        for (AttMap &m : att) m.valid = false;
    }

    // hipGraph replay of repeated forwards (same batch and the same caller buffers): the ~100 launches of a forward
    // become one graph launch.  Opt-in: measured on MI355X it does not change throughput (eager enqueue already runs
    // ahead of the GPU); what it saves is host time per forward.
    // A key is first run eagerly, captured on its second use, replayed from then on.
    typedef std::array<uintptr_t, 15> GraphKey;
    struct GraphEntry { GraphKey key; hipGraphExec_t exec; unsigned long long stamp; };
    bool graphs = false;
    // fused tail kernels (fusion_kernels.hip); HMV_NO_FFFUSE=1 / HMV_NO_CHEBFUSE=1 in the environment or hmv_set_tail_fusion(h, 0)
    // select the launch-per-op path (A/B runs, the equivalence test).  Part of the workspace plan: changing them re-plans.
    bool ff_fuse = true, cheb_fuse = true;
    bool hr_fuse = true;      // HRNet: the up-sampling terms of a fuse layer as one launch (hr_fuse.hip); hmv_set_hr_fusion(h, 0): one launch per term
    bool hr_overlap = true;   // HRNet, fp16-kernel modes: a module's lowest-resolution branch runs on a second stream beside the branch above it
                              // (hmv_set_hr_fusion bit 1; measured hr40 fp16 -1.2 %, f32x3 -0.9 %, fp32 +0.3 %: off in the fp32 mode)
    hipStream_t aux = nullptr;            // the second stream (forked from / joined into the caller's stream by events: also under graph capture)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool chain_fuse = true;   // conv3 -> next block's conv1 in one launch (conv_stream.hip chain); hmv_set_chain_fusion(h, 0) / HMV_NO_CHAIN=1
    std::vector<GraphEntry> gcache;
    std::vector<GraphKey> gseen;     // buffer sets run eagerly once and not captured yet (callers often alternate between a few)
    hipStream_t gstream = nullptr;   // capture happens here (the caller's stream may be the NULL stream, which cannot capture)
    unsigned long long gclock = 0, greplays = 0;
    void drop_graphs() {
        for (auto &e : gcache) (void)hipGraphExecDestroy(e.exec);
        gcache.clear();
        gseen.clear();
    }

    bool profiling = false;
    std::vector<ProfRec> prof;
    size_t prof_used = 0;
    int launches = 0;      // device operations (kernels, memsets, copies) enqueued by the last eager / captured forward
    // range word: every (hi, lo) pair conversion of a forward that clamps a value (|v| > 65504) sets it to 1 (note_range, kernels.h); sticky
    // until hmv_range_status reads it.  Its own allocation, outside the workspace arena: hmv_poison_workspace and cached graphs leave it alone
    int *sat = nullptr;

    int fail(int code, const char *fmt, ...) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return code;
    }
};

#define HIPCHK(h, expr)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess) return (h)->fail(HMV_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

namespace {

// ------------------------------------------------------------------ weight ingestion helpers
struct Loader {
    hmv_engine *h;
    int rc = HMV_OK;

    const HostTensor *get(const std::string &key, std::initializer_list<int64_t> shape) {
        auto it = h->host.find(key);
        if (it == h->host.end()) {
            if (rc == HMV_OK) rc = h->fail(HMV_ERR_MISSING_TENSOR, "Missing key(s) in state_dict: \"%s\"", key.c_str());
            return nullptr;
        }
        std::vector<int64_t> want(shape);
        if (it->second.shape != want) {
            if (rc == HMV_OK) {
                std::string got, exp;
                for (auto v : it->second.shape) got += std::to_string(v) + ",";
                for (auto v : want) exp += std::to_string(v) + ",";
                rc = h->fail(HMV_ERR_SHAPE, "size mismatch for %s: got [%s] expected [%s]", key.c_str(), got.c_str(), exp.c_str());
            }
            return nullptr;
        }
        return &it->second;
    }

    float *upload(const std::vector<float> &v) {
        if (rc != HMV_OK) return nullptr;
        float *p = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p), v.size() * sizeof(float));
        if (e == hipSuccess) e = hipMemcpy(p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            rc = h->fail(HMV_ERR_HIP, "weight upload failed: %s", hipGetErrorString(e));
            return nullptr;
        }
        h->dev_allocs.push_back(p);
        return p;
    }

    void *upload_bytes(const void *src, size_t bytes) {
        if (rc != HMV_OK) return nullptr;
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            rc = h->fail(HMV_ERR_HIP, "weight upload failed: %s", hipGetErrorString(e));
            return nullptr;
        }
        h->dev_allocs.push_back(p);
        return p;
    }

    // BatchNorm (eval) folded to scale/shift in double: resnet.py:59-74
    bool bn_fold(const std::string &prefix, int C, std::vector<double> &scale, std::vector<double> &shift) {
        const HostTensor *g = get(prefix + ".weight", {C}), *b = get(prefix + ".bias", {C});
        const HostTensor *rm = get(prefix + ".running_mean", {C}), *rv = get(prefix + ".running_var", {C});
        if (!g || !b || !rm || !rv) return false;
        scale.resize(C);
        shift.resize(C);
        for (int c = 0; c < C; ++c) {
            scale[c] = (double)g->data[c] / std::sqrt((double)rv->data[c] + 1e-5);
            shift[c] = (double)b->data[c] - (double)rm->data[c] * scale[c];
        }
        return true;
    }

    bool split = false;   // HMV_F32X3: fp16 layers carry [W_hi | W_hi | W_lo] against the activation sequence hi, lo, hi
    std::string src_key;  // the state_dict key(s) of the layer being packed (conv(): weight key + BatchNorm prefix), for errors

    // Generic finish: `wt(o, k)` supplies the un-scaled weight for output o, packed index k.
    template <typename F>
    void finish(Layer &L, const std::string &label, int Cin, int Cout, int R, int S, int K, F wt,
                const std::vector<double> *scale, const std::vector<double> *shift, const float *conv_bias, bool f16 = false,
                const std::vector<unsigned char> *lo_plane = nullptr) {
        L.label = label;
        L.Cin = Cin; L.Cout = Cout; L.R = R; L.S = S; L.K = K;
        L.f16 = f16;
        L.Kpad = round_up(K, f16 ? 64 : 32);
        L.Cout_pad = round_up(Cout, 256);
        if (rc != HMV_OK) return;
        std::vector<float> w((size_t)L.Cout_pad * L.Kpad, 0.f), b((size_t)L.Cout_pad, 0.f);
        for (int o = 0; o < Cout; ++o) {
            const double sc = scale ? (*scale)[o] : 1.0;
            for (int k = 0; k < K; ++k) w[(size_t)o * L.Kpad + k] = (float)((double)wt(o, k) * sc);
            double bb = shift ? (*shift)[o] : 0.0;
            if (conv_bias) bb += (double)conv_bias[o] * sc;
            b[o] = (float)bb;
        }
        if (f16 && !lo_plane) {   // plain fp16 storage: a folded weight past fp16's range would be packed as +-inf
            for (size_t i = 0; i < w.size(); ++i)
                if (!(std::fabs(w[i]) < 65520.f)) {
                    rc = h->fail(HMV_ERR_RANGE, "%s: folded weight %g (output channel %d) is outside the fp16 range (|w| < 65520)",
                                 src_key.empty() ? label.c_str() : src_key.c_str(), (double)w[i], (int)(i / L.Kpad));
                    return;
                }
        }
        if (f16) {   // BN scale is folded in fp32/double first, THEN rounded once to fp16
            std::vector<_Float16> wh(w.size());
            if (lo_plane) {   // split layers: scale by a power of two so that max |W| ~ 2^14 and W_lo stays a NORMAL fp16
                float mx = 0.f;
                for (float v : w) mx = std::max(mx, std::fabs(v));
                int sh = 0;
                while (sh < 24 && mx > 0.f && mx * 2.f <= 16384.f) { mx *= 2.f; ++sh; }
                while (sh > -24 && mx > 16384.f) { mx *= 0.5f; --sh; }   // huge folded weights (tiny running_var): scale down instead
                L.acc_shift = sh;
                const float f = std::ldexp(1.f, sh);
                for (float &v : w) v *= f;
            }
            for (size_t i = 0; i < w.size(); ++i) {
                const _Float16 hi = (_Float16)w[i];
                // split layers: packed index k of the third plane carries the residue W - fp16(W)
                wh[i] = (lo_plane && (*lo_plane)[i % (size_t)L.Kpad]) ? (_Float16)(w[i] - (float)hi) : hi;
            }
            L.w = static_cast<float *>(upload_bytes(wh.data(), wh.size() * sizeof(_Float16)));
        } else {
            L.w = upload(w);
        }
        L.bias = upload(b);
    }

    // nn.Conv2d weight OIHW (+ optional bias key) followed by an optional BN
    // (wsrc: an already re-arranged OIHW weight instead of the state_dict tensor `wkey` -- the space-to-depth stem)
    void conv(Layer &L, const std::string &label, const std::string &wkey, const std::string &bkey, const std::string &bn,
              int Cout, int Cin, int R, int S, int cin_pad = 0, bool f16 = false, bool rd = false, const float *wsrc = nullptr, bool tall = false) {
        const HostTensor *w = wsrc ? nullptr : get(wkey, {Cout, Cin, R, S});
        const HostTensor *cb = bkey.empty() ? nullptr : get(bkey, {Cout});
        src_key = wkey + (bn.empty() ? std::string() : " (folded with " + bn + ")");
        struct Clear { std::string &k; ~Clear() { k.clear(); } } clear_key{src_key};
        std::vector<double> sc, sh;
        const bool has_bn = !bn.empty();
        if (has_bn && !bn_fold(bn, Cout, sc, sh)) return;
        if ((!w && !wsrc) || (!bkey.empty() && !cb)) return;
        const int plane = cin_pad ? cin_pad : Cin;            // physical channels (per plane when split)
        const bool sp = split && f16;
        // fused split reduction: a k-step = 32 channels as [32 hi | 32 lo] halfs, K order (32-channel chunk, r, s, plane, c % 32)
        const bool x3n = sp && plane % 8 == 0 && !HMV_DEV_ENV("HMV_NO_X3N");
        const int cp = sp ? (x3n ? 2 * plane : 3 * plane) : plane;   // the channel count the kernel's K order walks
        const float *wd = wsrc ? wsrc : w->data.data();
        const bool chunked = cp % (f16 ? 64 : 32) == 0 && (!sp || (x3n && plane % 32 == 0) || (!x3n && plane % 64 == 0));
        tall = tall && f16 && !sp && !cin_pad && !rd && !wsrc;
        auto wt = [=](int o, int k) -> float {
            int c, tap;
            const int CH = (f16 && !tall) ? 64 : 32;
            if (x3n && chunked) {
                const int step = k / 64, c32 = k % 32;
                tap = step % (R * S);
                c = (step / (R * S)) * 32 + c32;
            } else if (x3n) {   // dense fused: 4 (tap, 8-channel) vectors per step, K order (r, s, c) over the real channels
                const int g = (k / 64) * 4 + (k % 32) / 8, cpt = plane / 8;
                tap = g / cpt;
                c = (g % cpt) * 8 + k % 8;
                if (tap >= R * S) return 0.f;
            } else if (chunked) {   // K order (chunk, r, s, c % CH), CH = 32 (fp32) / 64 (fp16): conv_igemm.hip
                const int chunk = k / (CH * R * S), rem = k % (CH * R * S);
                tap = rem / CH;
                c = chunk * CH + rem % CH;
            } else {          // dense K order (r, s, c) over the real channels: the stem, HRNet's 40 / 80-channel tensors
                c = k % cp;
                tap = k / cp;
            }
            if (sp && !x3n) c %= plane;   // virtual channel -> channel; which plane it is only decides hi / lo (lo_plane below)
            if (c >= Cin) return 0.f;
            return wd[(((size_t)o * Cin + c) * R + tap / S) * S + tap % S];
        };
        std::vector<unsigned char> lo_plane;
        // packed reduction length: the dense fused scheme packs 4 (tap, 8-channel) vectors per 64-wide step
        const int Kpack = (x3n && !chunked) ? (R * S * (plane / 8) + 3) / 4 * 64 : R * S * cp;
        if (sp) {   // packed indices whose virtual channel lies in the third plane
            const int K = Kpack, Kp = round_up(K, 64), CH = 64;
            lo_plane.assign(Kp, 0);
            for (int k = 0; k < K; ++k) {
                int c;
                if (x3n) { lo_plane[k] = (k % 64) >= 32; continue; }
                if (chunked) { const int chunk = k / (CH * R * S), rem = k % (CH * R * S); c = chunk * CH + rem % CH; }
                else c = k % cp;
                lo_plane[k] = c / plane == 2;
            }
        }
        if (rd && R == 3 && S == 3 && !cb && !sp) {
            // row-decomposed packing: GEMM output o' = (s, n), reduction k = (r, c); bias / BN shift live in group s = 0
            const int CH = f16 ? 64 : 32;
            auto wt3 = [=](int o2, int k) -> float {
                const int sx = o2 / Cout, n = o2 % Cout;
                int c, r;
                if (cp % CH == 0) {
                    const int chunk = k / (CH * 3), rem = k % (CH * 3);
                    r = rem / CH;
                    c = chunk * CH + rem % CH;
                } else {
                    c = k % cp;
                    r = k / cp;
                }
                if (c >= Cin) return 0.f;
                return wd[(((size_t)n * Cin + c) * 3 + r) * 3 + sx];
            };
            std::vector<double> sc3(3 * Cout, 1.0), sh3(3 * Cout, 0.0);
            for (int o2 = 0; o2 < 3 * Cout; ++o2) {
                if (has_bn) sc3[o2] = sc[o2 % Cout];
                if (has_bn && o2 < Cout) sh3[o2] = sh[o2];
            }
            finish(L, label, cp, 3 * Cout, 3, 1, 3 * cp, wt3, &sc3, &sh3, nullptr, f16);
            L.rd_cout = Cout;
            L.Kreal = 3 * Cin;   // (3 * Cout) x (3 * Cin) = Cout x 9 * Cin: the FLOP accounting sees the real convolution
            return;
        }
        finish(L, label, cp, Cout, R, S, Kpack, wt, has_bn ? &sc : nullptr, has_bn ? &sh : nullptr,
               cb ? cb->data.data() : nullptr, f16, sp ? &lo_plane : nullptr);
        L.Kreal = R * S * Cin;
        L.tall = tall;
        if (sp) { L.plane = plane; L.x3n = x3n; }
    }

    // nn.Linear weight [out][in] (+ optional bias)
    void linear(Layer &L, const std::string &label, const std::string &wkey, const std::string &bkey, int out, int in) {
        const HostTensor *w = get(wkey, {out, in});
        const HostTensor *b = bkey.empty() ? nullptr : get(bkey, {out});
        if (!w || (!bkey.empty() && !b)) return;
        const float *wd = w->data.data();
        auto wt = [=](int o, int k) -> float { return wd[(size_t)o * in + k]; };
        finish(L, label, round_up(in, 32), out, 1, 1, in, wt, nullptr, nullptr, b ? b->data.data() : nullptr);
    }

    // A bias-free fp32 linear on the fused split kernels (the fp16 / f32x3 modes' qkv projections): token rows arrive as
    // [hi plane | lo plane] halfs, a k-step is 32 columns as [32 W_hi | 32 W_lo]; fp32-equivalent, 3 fp16 MFMAs per fp32 one
    template <typename F>
    void linear_x3(Layer &L, const std::string &label, int plane, int out, int in, F wt) {
        auto wp = [=](int o, int k) -> float {
            const int c = (k / 64) * 32 + k % 32;
            return c < in ? wt(o, c) : 0.f;
        };
        std::vector<unsigned char> lo((size_t)2 * plane);
        for (int k = 0; k < 2 * plane; ++k) lo[k] = (k % 64) >= 32;
        finish(L, label, 2 * plane, out, 1, 1, 2 * plane, wp, nullptr, nullptr, nullptr, true, &lo);
        L.Kreal = in;
        L.plane = plane;
        L.x3n = true;
    }

    // Bottleneck conv3 and its block's downsample conv as ONE layer over the concatenated reduction [t2 | x] . [W3 ; Wds]
    // (resnet.py:124-144): a3 [outc][planes], ad [outc][inpl]; each half carries its own BN scale, the shifts add up.  Whole
    // 32 / 64-channel chunks on either side of the seam, else nothing is packed (-> false)
    bool conv_dual(Layer &L, const std::string &label, const float *a3, const float *ad, int planes, int inpl, int outc,
                   const std::vector<double> &s3, const std::vector<double> &b3, const std::vector<double> &sd_,
                   const std::vector<double> &bd_, bool h16) {
        const int CHK = h16 ? 64 : 32;
        if (planes % CHK != 0 || inpl % CHK != 0) return false;
        std::vector<double> shift(outc);
        for (int o = 0; o < outc; ++o) shift[o] = b3[o] + bd_[o];
        auto wt = [=, &s3, &sd_](int o, int k) -> double {
            return k < planes ? (double)a3[(size_t)o * planes + k] * s3[o] : (double)ad[(size_t)o * inpl + (k - planes)] * sd_[o];
        };
        finish(L, label, planes + inpl, outc, 1, 1, planes + inpl, wt, nullptr, &shift, nullptr, h16);
        L.Kreal = planes + inpl;
        return true;
    }

    // ConvTranspose2d(k4,s2,p1) weight wd [c0][cout][4][4] (+ bias cb, BN scale / shift) as 4 sub-pixel 2x2 convs dl[a * 2 + b]:
    // out[2q+a] takes ky = {3,1} (a=0, window starts at q-1) or {2,0} (a=1, window starts at q)
    void deconv_phases(Layer *dl, const std::string &label, const float *wd, const float *cb, int c0, int cout,
                       const std::vector<double> &sc, const std::vector<double> &sh, bool h16) {
        static const int kmap[2][2] = {{3, 1}, {2, 0}};
        for (int a = 0; a < 2; ++a)
            for (int b = 0; b < 2; ++b) {
                const int CH = h16 ? 64 : 32;
                const bool sp = split && h16;          // (hi, lo) pairs: the K order walks 3 * c0 virtual channels
                const int cv = sp ? 3 * c0 : c0;
                auto wt = [=](int o, int k) -> float {   // K order (chunk, r, s, c % CH)
                    const int chunk = k / (CH * 4), rem = k % (CH * 4), tap = rem / CH;
                    const int ci = (chunk * CH + rem % CH) % c0, r = tap / 2, s = tap % 2;
                    return wd[(((size_t)ci * cout + o) * 4 + kmap[a][r]) * 4 + kmap[b][s]];
                };
                std::vector<unsigned char> lo_plane;
                if (sp) {
                    lo_plane.assign(4 * cv, 0);
                    for (int k = 0; k < 4 * cv; ++k) lo_plane[k] = ((k / (CH * 4)) * CH + (k % (CH * 4)) % CH) / c0 == 2;
                }
                Layer &l = dl[a * 2 + b];
                finish(l, label + ".phase" + std::to_string(a * 2 + b), cv, cout, 2, 2, 4 * cv, wt,
                       &sc, &sh, cb, h16, sp ? &lo_plane : nullptr);
                l.Kreal = 4 * c0;
                if (sp) l.plane = c0;
            }
    }

    // the four phases' weight blocks back to back: one launch runs all of them (conv_igemm.hip, p.phases).  Not in the
    // split mode, whose per-layer power-of-two weight scale differs between the phases.  all.w stays null where it is not made
    void deconv_merge(const Layer *dl, Layer &all, size_t &stride, const std::string &label, bool h16) {
        all = Layer();
        if ((split && h16) || HMV_DEV_ENV("HMV_NO_PHASEMERGE") || rc != HMV_OK) return;
        const Layer &d0 = dl[0];
        const size_t elems = (size_t)d0.Cout_pad * d0.Kpad, bytes = elems * (h16 ? 2 : 4);
        void *blk = nullptr;
        hipError_t e = hipMalloc(&blk, 4 * bytes);
        for (int i = 0; i < 4 && e == hipSuccess; ++i)
            e = hipMemcpy(static_cast<char *>(blk) + i * bytes, dl[i].w, bytes, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) rc = h->fail(HMV_ERR_HIP, "weight upload failed: %s", hipGetErrorString(e));
        if (blk) h->dev_allocs.push_back(blk);
        if (e == hipSuccess) {
            all = d0;
            all.label = label;
            all.w = static_cast<float *>(blk);
            stride = elems;
        }
    }

    float *vec(const std::string &key, int n) {
        const HostTensor *t = get(key, {n});
        return t ? upload(t->data) : nullptr;
    }
};

int backbone_level_channels(const hmv_config &c, int level /*0 = layer1*/) {
    return (64 << level) * (c.backbone == HMV_RESNET50_PAPER ? 4 : 1);
}

}  // namespace

// ====================================================================== C ABI
extern "C" {

const char *hmv_version(void) {
#ifdef HMV_DEV_KNOBS
    return "handmv-mi355x 0.4-dev (gfx950; arithmetic modes: f32 = native fp32 MFMA, f16 = fp16 storage + fp16 MFMA with fp32 accumulation, "
           "f32x3 = (hi, lo) fp16 pairs on the fp16 MFMA, fp32-equivalent; development knobs compiled in)";
#else
    return "handmv-mi355x 0.4 (gfx950; arithmetic modes: f32 = native fp32 MFMA, f16 = fp16 storage + fp16 MFMA with fp32 accumulation, "
           "f32x3 = (hi, lo) fp16 pairs on the fp16 MFMA, fp32-equivalent)";
#endif
}

// The tile conv_igemm's launcher rule gives a conv / GEMM of M output pixels, Cout channels and reduction length K ("256x256", "128x32",
// "256x128,k16,w8" ...): host logic only, no GPU call -- the CPU tests pin the rules that were measured on the hardware.
const char *hmv_tile_rule(int32_t M, int32_t Cout, int32_t K, int32_t f16, int32_t has_residual) {
    const ConvTile t = conv_pick_tile(M, Cout, K, f16 != 0, has_residual != 0);
    const char *n = f16 ? conv_tile_name_f16(t, 0) : conv_tile_name(t, 0);   // "conv_igemm_f32<256x256,taps>"
    static thread_local char buf[64];
    const char *lt = strchr(n, '<'), *comma = lt ? strrchr(n, ',') : nullptr;
    if (!lt || !comma || comma < lt) return n;
    const size_t len = (size_t)(comma - lt - 1) < sizeof(buf) - 1 ? (size_t)(comma - lt - 1) : sizeof(buf) - 1;
    memcpy(buf, lt + 1, len);
    buf[len] = 0;
    return buf;
}

const char *hmv_last_error(hmv_handle h) { return h ? h->err.c_str() : g_create_err.c_str(); }

// the handle-less entries of the other translation units (losses.hip) report through the same per-thread text
extern "C++" void hmv::set_thread_error(const std::string &msg) { g_create_err = msg; }

int hmv_create(const hmv_config *cfg, hmv_handle *out) {
    auto bad = [&](const char *m) { g_create_err = m; return HMV_ERR_ARG; };
    if (!cfg || !out) return bad("null argument");
    if (cfg->struct_size != (int32_t)sizeof(hmv_config)) return bad("hmv_config.struct_size mismatch (ABI)");
    if (cfg->backbone < HMV_RESNET18 || cfg->backbone > HMV_HRNET_W64) return bad("Supports only 18, 34, 50_paper (resnet) and w40, w64 (hrnet)");
    if (cfg->num_views < 1 || cfg->num_views > 48) return bad("num_views must be in [1, 48]");
    if (cfg->fusion != HMV_FUSION_CROSS_ATTN && cfg->fusion != HMV_FUSION_LEARNABLE_QUERY) return bad("Invalid fusion type");
    if (cfg->fusion == HMV_FUSION_CROSS_ATTN && (cfg->fusion_layers < 1 || cfg->fusion_layers % 2 != 1))
        return bad("num_layers must be an odd number");
    if (cfg->dtype != HMV_F32 && cfg->dtype != HMV_F16 && cfg->dtype != HMV_F32X3) { g_create_err = "dtype must be HMV_F32, HMV_F16 or HMV_F32X3"; return HMV_ERR_UNSUPPORTED; }
    // ResNet backbones take any frame size the reference's convs take (resnet.py:216-254); HRNet's fuse layers add 2^k-upsampled
    // maps (hrnet.py:194-212), which only line up -- in the reference as here -- when every branch size is exact
    if (cfg->height < 32 || cfg->width < 32) return bad("frame height/width must be at least 32");
    if (cfg->backbone >= HMV_HRNET_W40 && (cfg->height % 32 || cfg->width % 32))
        return bad("HRNet frame height/width must be multiples of 32 (its fuse layers need exact 2x branch sizes)");
    if (cfg->image_size <= 0 || cfg->heatmap_size <= 0) return bad("image_size / heatmap_size must be positive");
    const bool paper = cfg->backbone == HMV_RESNET50_PAPER;
    const bool hrnet = cfg->backbone >= HMV_HRNET_W40;
    if (cfg->n_levels < 1 || cfg->n_levels > (hrnet ? 4 : (paper ? 1 : 3))) return bad("backbone_channels has too many levels for this backbone");
    for (int i = 0; i < cfg->n_levels; ++i)
        if (cfg->channels[i] != (hrnet ? kHrChannels[cfg->backbone - HMV_HRNET_W40][i] : backbone_level_channels(*cfg, 2 - i)))
            return bad("backbone_channels do not match the backbone");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        g_create_err = "no HIP device: libhandmv has no CPU fallback";
        return HMV_ERR_HIP;
    }
    if (cfg->device < 0 || cfg->device >= ndev) return bad("device ordinal out of range");
    hmv_engine *h = new hmv_engine();
    {   // the range word, on the handle's device (the calling thread's current device is left as it was)
        int prev = 0;
        hipError_t e = hipGetDevice(&prev);
        if (e == hipSuccess) e = hipSetDevice(cfg->device);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&h->sat), sizeof(int));
        if (e == hipSuccess) e = hipMemset(h->sat, 0, sizeof(int));
        if (e == hipSuccess) e = hipDeviceSynchronize();
        (void)hipSetDevice(prev);
        if (e != hipSuccess) {
            g_create_err = std::string("range word allocation failed: ") + hipGetErrorString(e);
            if (h->sat) (void)hipFree(h->sat);
            delete h;
            return HMV_ERR_HIP;
        }
    }
    if (const char *g = getenv("HMV_GRAPHS")) h->graphs = atoi(g) != 0;
    h->ff_fuse = HMV_DEV_ENV("HMV_NO_FFFUSE") == nullptr;
    h->cheb_fuse = HMV_DEV_ENV("HMV_NO_CHEBFUSE") == nullptr;
    h->cfg = *cfg;
    h->paper = paper;
    h->hrnet = hrnet;
    h->lq = cfg->fusion == HMV_FUSION_LEARNABLE_QUERY;
    h->fdim = 0;
    for (int i = 0; i < cfg->n_levels; ++i) h->fdim += cfg->channels[i] / 2;
    h->d = h->fdim + ((cfg->pos_enc & HMV_POS2D) ? 2 : 0) + ((cfg->pos_enc & HMV_POS_CROP) ? 10 : 0);
    h->ldt = round_up(h->d, 32);
    *out = h;
    return HMV_OK;
}

int hmv_set_tensor(hmv_handle h, const char *key, const float *host, const int64_t *shape, int32_t ndim) {
    if (!h || !key || !host || ndim < 0 || ndim > 4) return h ? h->fail(HMV_ERR_ARG, "bad hmv_set_tensor argument") : HMV_ERR_ARG;
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) { t.shape.push_back(shape[i]); n *= (size_t)shape[i]; }
    t.data.assign(host, host + n);
    h->host[key] = std::move(t);
    h->finalized = false;
    return HMV_OK;
}

int hmv_finalize_weights(hmv_handle h) {
    if (!h) return HMV_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    // re-finalisation: forwards in flight and captured graphs still point at the old weight buffers
    HIPCHK(h, hipDeviceSynchronize());
    h->drop_graphs();
    h->finalized = false;
    for (void *p : h->dev_allocs) (void)hipFree(p);
    h->dev_allocs.clear();
    for (auto &v : h->blocks) v.clear();
    h->attn.clear();
    Loader L{h};
    const hmv_config &c = h->cfg;
    const int exp = h->paper ? 4 : 1;
    const bool h16 = c.dtype != HMV_F32;   // conv stack on the fp16 kernels; heat-map logits, tokens, fusion, decoder stay fp32
    L.split = c.dtype == HMV_F32X3;        // ... with (hi, lo) pairs: fp32-equivalent

    if (h->hrnet) {
        // ---- HighResolutionNet: hrnet.py:231-311.  Every tensor keeps its real channel stride (dense-K conv mode for 40 / 80 channels).
        HrNet &hr = h->hr;
        hr = HrNet();
        for (int i = 0; i < 4; ++i) hr.ch[i] = kHrChannels[c.backbone - HMV_HRNET_W40][i];
        // the highest-resolution branch (H/4 x W/4) of w40 has 40 channels: its stride-1 3x3 convs run row-decomposed
        // when a 128-row tile covers whole image rows (conv_igemm.hip, RD)
        // (only where it removes padding: channel counts that are not multiples of 32, i.e. w40's 40- and 80-wide branches)
        bool rdb[4] = {false, false, false, false};
        for (int b = 0; b < 2; ++b)
            rdb[b] = 3 * hr.ch[b] <= 256 && hr.ch[b] % 32 != 0 && hr.ch[b] % 4 == 0 && 128 % (c.width / (4 << b)) == 0 && !L.split &&
                     !HMV_DEV_ENV("HMV_NO_ROWSUM");
        // fp16 path, 40-channel branch on frames whose H/4 x W/4 map tiles into 16 x 16 blocks: plain (r, s, c) packing instead, so
        // that the weight-stationary halo-streaming kernel (conv_hs.hip: 1.9 -> ~4 TB/s on these layers) takes the large batches
        // and conv_igemm's dense mode -- same K order, same bits -- the small ones.  Decided by the configuration, never by the batch.
        if (h16 && !L.split && hr.ch[0] == 40 && c.height % 64 == 0 && c.width % 64 == 0 && !HMV_DEV_ENV("HMV_NO_HS")) rdb[0] = false;
        // ... and the 80-channel branch (H/8 x W/8 maps in 8 x 16 blocks; conv_hs.hip's three-wave variant)
        if (h16 && !L.split && hr.ch[1] == 80 && c.height % 64 == 0 && c.width % 128 == 0 && !HMV_DEV_ENV("HMV_NO_HS") && !HMV_DEV_ENV("HMV_NO_HS80")) rdb[1] = false;
        const bool rd0 = rdb[0];
        L.conv(hr.conv1, "stem.conv1", "backbone.conv1.weight", "", "backbone.bn1", 64, 3, 3, 3, /*cin_pad=*/h16 ? 8 : 4, h16);
        L.conv(hr.conv2, "stem.conv2", "backbone.conv2.weight", "", "backbone.bn2", 64, 64, 3, 3, 0, h16);
        int inpl_ = 64;
        for (int bi = 0; bi < 4; ++bi) {
            Block b;
            const std::string p = "backbone.layer1." + std::to_string(bi), lab = "layer1." + std::to_string(bi);
            L.conv(b.c1, lab + ".conv1", p + ".conv1.weight", "", p + ".bn1", 64, inpl_, 1, 1, 0, h16);
            L.conv(b.c2, lab + ".conv2", p + ".conv2.weight", "", p + ".bn2", 64, 64, 3, 3, 0, h16);
            L.conv(b.c3, lab + ".conv3", p + ".conv3.weight", "", p + ".bn3", 256, 64, 1, 1, 0, h16);
            b.has_ds = bi == 0;
            if (b.has_ds) L.conv(b.ds, lab + ".downsample", p + ".downsample.0.weight", "", p + ".downsample.1", 256, 64, 1, 1, 0, h16);
            inpl_ = 256;
            hr.layer1.push_back(b);
        }
        static const int NMOD[3] = {1, 4, 3};
        int npre = 1, prec[4] = {256, 0, 0, 0};
        for (int st = 0; st < 3; ++st) {
            const int nbr = st + 2;
            const std::string tp = "backbone.transition" + std::to_string(st + 1);
            for (int i = 0; i < nbr; ++i) {   // _make_transition_layer: hrnet.py:287-311
                hr.trans[st][i].clear();
                if (i < npre) {
                    if (hr.ch[i] != prec[i]) {
                        Layer l;
                        const std::string q = tp + "." + std::to_string(i);
                        L.conv(l, "transition" + std::to_string(st + 1) + "." + std::to_string(i), q + ".0.weight", "", q + ".1",
                               hr.ch[i], prec[i], 3, 3, cpad(prec[i]), h16, i == 0 && rd0);
                        hr.trans[st][i].push_back(l);
                    }
                } else {
                    int cin = prec[npre - 1];
                    for (int j = 0; j < i + 1 - npre; ++j) {
                        const int outc = (j == i - npre) ? hr.ch[i] : cin;
                        Layer l;
                        const std::string q = tp + "." + std::to_string(i) + "." + std::to_string(j);
                        L.conv(l, "transition" + std::to_string(st + 1) + "." + std::to_string(i) + "." + std::to_string(j),
                               q + ".0.weight", "", q + ".1", outc, cin, 3, 3, cpad(cin), h16);
                        hr.trans[st][i].push_back(l);
                        cin = outc;
                    }
                }
            }
            hr.stage[st].clear();
            for (int m = 0; m < NMOD[st]; ++m) {
                hr.stage[st].emplace_back();
                HrModule &M = hr.stage[st].back();
                const std::string mp = "backbone.stage" + std::to_string(st + 2) + "." + std::to_string(m);
                const std::string ml = "stage" + std::to_string(st + 2) + "." + std::to_string(m);
                for (int b = 0; b < nbr; ++b)
                    for (int blk = 0; blk < 4; ++blk) {
                        const std::string bp = mp + ".branches." + std::to_string(b) + "." + std::to_string(blk);
                        const std::string bl = ml + ".b" + std::to_string(b) + "." + std::to_string(blk);
                        L.conv(M.br[b][blk][0], bl + ".conv1", bp + ".conv1.weight", "", bp + ".bn1", hr.ch[b], hr.ch[b], 3, 3, cpad(hr.ch[b]), h16, rdb[b]);
                        L.conv(M.br[b][blk][1], bl + ".conv2", bp + ".conv2.weight", "", bp + ".bn2", hr.ch[b], hr.ch[b], 3, 3, cpad(hr.ch[b]), h16, rdb[b]);
                    }
                for (int i = 0; i < nbr; ++i)
                    for (int j = 0; j < nbr; ++j) {
                        const std::string fp = mp + ".fuse_layers." + std::to_string(i) + "." + std::to_string(j);
                        const std::string fl = ml + ".fuse" + std::to_string(i) + std::to_string(j);
                        if (j > i) {
                            Layer l;
                            L.conv(l, fl, fp + ".0.weight", "", fp + ".1", hr.ch[i], hr.ch[j], 1, 1, cpad(hr.ch[j]), h16);
                            M.fuse[i][j].push_back(l);
                            if (h16 && !L.split && nbr - 1 - i >= 2)   // (only branches with two or more up-sampling terms run fused)
                                L.conv(M.fup[i][j], fl, fp + ".0.weight", "", fp + ".1", hr.ch[i], hr.ch[j], 1, 1, cpad(hr.ch[j]), false);
                        } else if (j < i) {
                            for (int q = 0; q < i - j; ++q) {
                                const int outc = (q == i - j - 1) ? hr.ch[i] : hr.ch[j];
                                Layer l;
                                const std::string fq = fp + "." + std::to_string(q);
                                L.conv(l, fl + "." + std::to_string(q), fq + ".0.weight", "", fq + ".1", outc, hr.ch[j], 3, 3, cpad(hr.ch[j]), h16);
                                M.fuse[i][j].push_back(l);
                            }
                        }
                    }
            }
            npre = nbr;
            for (int i = 0; i < nbr; ++i) prec[i] = hr.ch[i];
        }
        // pose_net = nn.Conv2d(C0, 21, 3, stride 2, padding 1): handmvnet.py:51-57
        L.conv(h->pose0, "pose_net", "pose_net.weight", "pose_net.bias", "", NJ, c.channels[0], 3, 3, cpad(c.channels[0]), h16);
    } else {
    // ---- backbone: resnet.py:162-177, 189-203
    {   // conv1 7x7 s2 p3 as the 4x4 s1 p2 conv over the 2x2 space-to-depth image (misc_kernels.hip, nchw_to_s2d_kernel):
        // kernel row r reads input row 2y - 3 + r = row pair y - 2 + (r + 1) / 2, sub-row (r + 1) % 2; s2d channel (dy, dx, c)
        const HostTensor *w7 = L.get("backbone.conv1.weight", {64, 3, 7, 7});
        std::vector<float> ws((size_t)64 * 12 * 16, 0.f);
        if (w7)
            for (int o = 0; o < 64; ++o)
                for (int c = 0; c < 3; ++c)
                    for (int r = 0; r < 7; ++r)
                        for (int q = 0; q < 7; ++q) {
                            const int ty = (r + 1) >> 1, dy = (r + 1) & 1, tx = (q + 1) >> 1, dx = (q + 1) & 1;
                            ws[(((size_t)o * 12 + (dy * 2 + dx) * 3 + c) * 4 + ty) * 4 + tx] = w7->data[(((size_t)o * 3 + c) * 7 + r) * 7 + q];
                        }
        L.conv(h->stem, "stem", "", "", "backbone.bn1", 64, 12, 4, 4, /*cin_pad=*/h16 ? 16 : 12, h16, false, ws.data());
        h->stem.Kreal = 7 * 7 * 3;   // FLOP / byte accounting sees the real convolution
        h->stem.in_real = 12;        // real input elements per (s2d) input pixel
    }
    int inpl = 64;
    for (int li = 0; li < 3; ++li) {
        const int planes = 64 << li;
        int stride = li == 0 ? 1 : 2;
        if (h->paper && li == 2) stride = 1;
        for (int bi = 0; bi < kBlocks[c.backbone][li]; ++bi) {
            Block b;
            b.stride = bi == 0 ? stride : 1;
            const std::string p = "backbone.layer" + std::to_string(li + 1) + "." + std::to_string(bi);
            const std::string lab = "layer" + std::to_string(li + 1) + "." + std::to_string(bi);
            const int outc = planes * exp;
            if (h->paper) {
                L.conv(b.c1, lab + ".conv1", p + ".conv1.weight", "", p + ".bn1", planes, inpl, 1, 1, 0, h16);
                // conv2 at stride 1 on a map that tiles into 16 x 32 blocks: the tall-tile kernel (conv_ht.hip), chosen by the
                // configuration alone -- the map is H/8 x W/8 from layer2.1 on (layer3 keeps it: the paper variant's stride 1)
                auto hup = [](int n) { return (n - 1) / 2 + 1; };
                const int mh = hup(hup(hup(c.height))), mw = hup(hup(hup(c.width)));
                const bool tall = h16 && li >= 1 && b.stride == 1 && conv_ht_shape_ok(3, 3, 1, 1, planes, planes, mh, mw);
                L.conv(b.c2, lab + ".conv2", p + ".conv2.weight", "", p + ".bn2", planes, planes, 3, 3, 0, h16, false, nullptr, tall);
                L.conv(b.c3, lab + ".conv3", p + ".conv3.weight", "", p + ".bn3", outc, planes, 1, 1, 0, h16);
            } else {
                L.conv(b.c1, lab + ".conv1", p + ".conv1.weight", "", p + ".bn1", planes, inpl, 3, 3, 0, h16);
                L.conv(b.c2, lab + ".conv2", p + ".conv2.weight", "", p + ".bn2", planes, planes, 3, 3, 0, h16);
            }
            b.has_ds = (b.stride != 1 || inpl != outc);
            if (b.has_ds) L.conv(b.ds, lab + ".downsample", p + ".downsample.0.weight", "", p + ".downsample.1", outc, inpl, 1, 1, 0, h16);
            static const bool no_fuse = HMV_DEV_ENV("HMV_NO_DSFUSE") != nullptr;   // development knob (A/B runs)
            if (b.has_ds && h->paper && !L.split && !no_fuse) {
                const int CHK = h16 ? 64 : 32;
                const HostTensor *w3 = L.get(p + ".conv3.weight", {outc, planes, 1, 1}), *wd = L.get(p + ".downsample.0.weight", {outc, inpl, 1, 1});
                std::vector<double> s3, b3, sd_, bd_;
                if (w3 && wd && planes % CHK == 0 && inpl % CHK == 0 && L.bn_fold(p + ".bn3", outc, s3, b3) &&
                    L.bn_fold(p + ".downsample.1", outc, sd_, bd_))
                    b.fused_ds = L.conv_dual(b.c3ds, lab + ".conv3+downsample", w3->data.data(), wd->data.data(), planes, inpl, outc,
                                             s3, b3, sd_, bd_, h16);
            }
            inpl = outc;
            h->blocks[li].push_back(b);
        }
    }
    // ---- pose_net: handmvnet.py:70-86
    const int c0 = c.channels[0];
    if (h->paper) {
        L.conv(h->pose0, "pose_net.0", "pose_net.0.weight", "pose_net.0.bias", "pose_net.1", 512, c0, 1, 1, 0, h16);
        L.conv(h->pose1, "pose_net.3", "pose_net.3.weight", "pose_net.3.bias", "", NJ, 512, 1, 1, 0, h16);
    } else {
        // ConvTranspose2d(k4,s2,p1) weight [Cin][Cout][4][4] as 4 sub-pixel 2x2 convs:
        // out[2q+a] takes ky = {3,1} (a=0, window starts at q-1) or {2,0} (a=1, window starts at q)
        const HostTensor *w = L.get("pose_net.0.weight", {c0, 128, 4, 4});
        const HostTensor *cb = L.get("pose_net.0.bias", {128});
        std::vector<double> sc, sh;
        const bool ok = L.bn_fold("pose_net.1", 128, sc, sh);
        if (w && cb && ok) {
            L.deconv_phases(h->deconv, "pose_net.0", w->data.data(), cb->data.data(), c0, 128, sc, sh, h16);
            L.deconv_merge(h->deconv, h->deconv_all, h->deconv_stride, "pose_net.0", h16);
        }
        L.conv(h->pose1, "pose_net.3", "pose_net.3.weight", "pose_net.3.bias", "pose_net.4", 64, 128, 3, 3, 0, h16);
        L.conv(h->pose2, "pose_net.6", "pose_net.6.weight", "pose_net.6.bias", "", NJ, 64, 3, 3, 0, h16);
    }
    }   // resnet backbones
    // ---- sample nets: nets.py:24-31
    for (int i = 0; i < c.n_levels; ++i) {
        const std::string p = "sample_nets." + std::to_string(i) + ".conv";
        L.conv(h->sample[i], "sample_nets." + std::to_string(i), p + ".0.weight", p + ".0.bias", p + ".1", c.channels[i] / 2,
               c.channels[i], 1, 1, h->hrnet ? cpad(c.channels[i]) : 0, h16);
    }
    // ---- fusion: layers.py:177-200
    const int d = h->d;
    // sinusoidal PE table (plain attribute in the reference, not in the state_dict): layers.py:134-158.  The learnable-query
    // blocks carry their own pos_embed and always add it.
    std::vector<float> pe_host;
    if ((c.pos_enc & HMV_POS_SIN) || h->lq) {
        const int T = c.num_views * NJ;
        pe_host.resize((size_t)T * d);
        for (int p = 0; p < T; ++p)
            for (int cc = 0; cc < d; ++cc) {
                const int k2 = cc & ~1;
                const float div = expf((float)k2 * (float)(-std::log(10000.0) / (double)d));
                const float ang = (float)p * div;
                pe_host[(size_t)p * d + cc] = (cc & 1) ? cosf(ang) : sinf(ang);
            }
        h->pe = L.upload(pe_host);
    } else {
        h->pe = nullptr;
    }
    // fp16 / f32x3 modes: the q/k/v projections (the fusion stage's largest GEMMs) run on the fused split fp16 kernels --
    // fp32-equivalent results at a third of the fp32 MFMA time.  Chosen by dtype alone, never by the batch.
    const bool x3lin = h16 && !HMV_DEV_ENV("HMV_NO_X3LIN");
    if (h->lq) {
        // CrossAttentionFusionLearnableQuery: fusion.py:33-49; MultiHeadAttentionLearnableQuery: layers.py:240-301
        for (int l = 0; l < 5; ++l) {
            AttnLayer a;
            const std::string p = "joints_late_fusion.attn_fusion." + std::to_string(l);
            const std::string lab = "fusion_lq." + std::to_string(l);
            const bool cross = l == 2;
            const HostTensor *wq = L.get(p + ".to_q.weight", {INNER_LQ, d}), *wk = L.get(p + ".to_k.weight", {INNER_LQ, d}),
                             *wv = L.get(p + ".to_v.weight", {INNER_LQ, d});
            if (wq && wk && wv) {
                const float *q = wq->data.data(), *k = wk->data.data(), *v = wv->data.data();
                if (cross) {
                    auto wt = [=](int o, int kk) -> float { return (o < INNER_LQ ? k : v)[(size_t)(o % INNER_LQ) * d + kk]; };
                    if (x3lin) L.linear_x3(a.kv, lab + ".kv", h->ldt, 2 * INNER_LQ, d, wt);
                    else L.finish(a.kv, lab + ".kv", h->ldt, 2 * INNER_LQ, 1, 1, d, wt, nullptr, nullptr, nullptr);
                    const HostTensor *pr = L.get(p + ".probe", {1, NJ, d});
                    if (pr) {   // q = to_q(probe + pe[:21]) in double, once
                        std::vector<float> qp((size_t)NJ * INNER_LQ);
                        for (int t = 0; t < NJ; ++t)
                            for (int o = 0; o < INNER_LQ; ++o) {
                                double acc = 0.0;
                                for (int kk = 0; kk < d; ++kk)
                                    acc += (double)(pr->data[(size_t)t * d + kk] + pe_host[(size_t)t * d + kk]) * (double)q[(size_t)o * d + kk];
                                qp[(size_t)t * INNER_LQ + o] = (float)acc;
                            }
                        a.qprobe = L.upload(qp);
                    }
                } else {
                    auto wt = [=](int o, int kk) -> float {
                        const float *src = o < INNER_LQ ? q : (o < 2 * INNER_LQ ? k : v);
                        return src[(size_t)(o % INNER_LQ) * d + kk];
                    };
                    if (x3lin) L.linear_x3(a.qkv, lab + ".qkv", h->ldt, 3 * INNER_LQ, d, wt);
                    else L.finish(a.qkv, lab + ".qkv", h->ldt, 3 * INNER_LQ, 1, 1, d, wt, nullptr, nullptr, nullptr);
                }
            }
            L.linear(a.out, lab + ".to_out", p + ".to_out.0.weight", p + ".to_out.0.bias", d, INNER_LQ);
            if (x3lin) {   // fp16-kernel modes: to_out once more as a split-pair GEMM (gemm_x3.hip), as in CrossAttentionFusion below
                const HostTensor *wo = L.get(p + ".to_out.0.weight", {d, INNER_LQ});
                if (wo) {
                    const float *o_ = wo->data.data();
                    L.linear_x3(a.out_x3, lab + ".to_out", INNER_LQ, d, INNER_LQ, [=](int o, int kk) -> float { return o_[(size_t)o * INNER_LQ + kk]; });
                }
            }
            L.linear(a.ff1, lab + ".ff1", p + ".ff.net.1.weight", p + ".ff.net.1.bias", DHEAD_LQ, d);
            L.linear(a.ff2, lab + ".ff2", p + ".ff.net.4.weight", p + ".ff.net.4.bias", d, DHEAD_LQ);
            a.fg = L.vec(p + ".ff.net.0.weight", d); a.fb = L.vec(p + ".ff.net.0.bias", d);
            h->attn.push_back(a);
        }
    }
    for (int l = 0; l < (h->lq ? 0 : c.fusion_layers); ++l) {
        AttnLayer a;
        const std::string p = "joints_late_fusion.attn_fusion." + std::to_string(l);
        const std::string lab = "fusion." + std::to_string(l);
        const HostTensor *wq = L.get(p + ".to_q.weight", {INNER, d}), *wk = L.get(p + ".to_k.weight", {INNER, d}),
                         *wv = L.get(p + ".to_v.weight", {INNER, d});
        if (wq && wk && wv) {
            const float *q = wq->data.data(), *k = wk->data.data(), *v = wv->data.data();
            auto wt = [=](int o, int kk) -> float {
                const float *src = o < INNER ? q : (o < 2 * INNER ? k : v);
                return src[(size_t)(o % INNER) * d + kk];
            };
            if (x3lin) L.linear_x3(a.qkv, lab + ".qkv", h->ldt, 3 * INNER, d, wt);
            else L.finish(a.qkv, lab + ".qkv", h->ldt, 3 * INNER, 1, 1, d, wt, nullptr, nullptr, nullptr);
        }
        L.linear(a.out, lab + ".to_out", p + ".to_out.weight", p + ".to_out.bias", d, INNER);
        if (x3lin) {
            const HostTensor *wo = L.get(p + ".to_out.weight", {d, INNER});
            if (wo) {
                const float *o_ = wo->data.data();
                L.linear_x3(a.out_x3, lab + ".to_out", INNER, d, INNER, [=](int o, int kk) -> float { return o_[(size_t)o * INNER + kk]; });
            }
        }
        L.linear(a.ff1, lab + ".ff1", p + ".ff.net.1.weight", p + ".ff.net.1.bias", DHEAD, d);
        L.linear(a.ff2, lab + ".ff2", p + ".ff.net.4.weight", p + ".ff.net.4.bias", d, DHEAD);
        a.n1g = L.vec(p + ".norm1.weight", d); a.n1b = L.vec(p + ".norm1.bias", d);
        a.n2g = L.vec(p + ".norm2.weight", d); a.n2b = L.vec(p + ".norm2.bias", d);
        a.fg = L.vec(p + ".ff.net.0.weight", d); a.fb = L.vec(p + ".ff.net.0.bias", d);
        h->attn.push_back(a);
    }
    // ---- decoder: nets.py:119-154
    if (c.decoder == HMV_DECODER_GCN) {
        const int dims[4] = {d, 256, 64, 3};
        for (int i = 0; i < 3; ++i) {
            const std::string p = "joints_decoder.joints_gcn" + std::to_string(i + 1);
            const int ci = dims[i], co = dims[i + 1];
            const HostTensor *w = L.get(p + ".weight", {3, 1, ci, co});
            const HostTensor *b = L.get(p + ".bias", {1, 1, co});
            if (w && b) {
                const float *wd = w->data.data();
                auto wt = [=](int o, int k) -> float { return wd[((size_t)(o / co) * ci + k) * co + (o % co)]; };
                L.finish(h->gcn[i], "decoder.gcn" + std::to_string(i + 1), round_up(ci, 32), 3 * co, 1, 1, ci, wt, nullptr,
                         nullptr, nullptr);
                h->gcn_bias[i] = L.upload(b->data);
            }
        }
        // Chebyshev polynomials of the fixed hand graph: utils.py:108-120, layers.py:405-445, constants.py:37-41
        static const int E[20][2] = {{0, 1}, {1, 2}, {2, 3}, {3, 4}, {0, 5}, {5, 6}, {6, 7}, {7, 8}, {0, 9}, {9, 10},
                                     {10, 11}, {11, 12}, {0, 13}, {13, 14}, {14, 15}, {15, 16}, {0, 17}, {17, 18},
                                     {18, 19}, {19, 20}};
        float adj[NJ][NJ] = {}, Lp[NJ][NJ];
        for (auto &e : E) { adj[e[0]][e[1]] = 1.f; adj[e[1]][e[0]] = 1.f; }
        for (int i = 0; i < NJ; ++i) adj[i][i] += 1.f;
        for (int i = 0; i < NJ; ++i) {
            float rs = 0.f;
            for (int j = 0; j < NJ; ++j) rs += adj[i][j];
            const float inv = rs != 0.f ? 1.f / rs : 0.f;
            for (int j = 0; j < NJ; ++j) adj[i][j] *= inv;
        }
        float dsq[NJ];
        for (int i = 0; i < NJ; ++i) {
            float rs = 0.f;
            for (int j = 0; j < NJ; ++j) rs += adj[i][j];
            dsq[i] = 1.f / std::sqrt(rs);
        }
        std::vector<float> tk(3 * NJ * NJ);
        for (int i = 0; i < NJ; ++i)
            for (int j = 0; j < NJ; ++j) {
                Lp[i][j] = (i == j ? 1.f : 0.f) - dsq[i] * adj[i][j] * dsq[j];
                tk[(0 * NJ + i) * NJ + j] = i == j ? 1.f : 0.f;
                tk[(1 * NJ + i) * NJ + j] = Lp[i][j];
            }
        for (int i = 0; i < NJ; ++i)
            for (int j = 0; j < NJ; ++j) {
                float s = 0.f;
                for (int m = 0; m < NJ; ++m) s += Lp[i][m] * Lp[m][j];
                tk[(2 * NJ + i) * NJ + j] = 2.f * s - (i == j ? 1.f : 0.f);
            }
        h->cheb_t = L.upload(tk);
    } else {
        L.linear(h->fc1, "decoder.fc1", "joints_decoder.joints_fc1.weight", "joints_decoder.joints_fc1.bias", 64, d);
        L.linear(h->fc2, "decoder.fc2", "joints_decoder.joints_fc2.weight", "joints_decoder.joints_fc2.bias", 3, 64);
    }
    h->zero_bias = L.upload(std::vector<float>(4096, 0.f));
    if (L.rc != HMV_OK) return L.rc;
    HIPCHK(h, hipDeviceSynchronize());
    h->finalized = true;
    h->host.clear();  // host copies are no longer needed
    return HMV_OK;
}


// Diagnostic: time `iters` launches of one conv shape with a chosen tile (tile < 0: engine's choice).
// HMV_BENCH_DTYPE=f16 in the environment runs the shape on the fp16 kernels (fp16 activations / weights / residual / output).
int hmv_bench_conv(int32_t device, int32_t N, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t R, int32_t S,
                   int32_t stride, int32_t pad, int32_t with_residual, int32_t tile, int32_t iters, float *avg_ms) {
    if (hipSetDevice(device) != hipSuccess) return HMV_ERR_HIP;
    const char *edt = HMV_DEV_ENV("HMV_BENCH_DTYPE");
    const bool f16 = edt && std::string(edt) == "f16";
    const size_t eb = f16 ? 2 : 4;
    const int Ho = (H + 2 * pad - R) / stride + 1, Wo = (W + 2 * pad - S) / stride + 1;
    const int K = R * S * Cin, Kpad = round_up(K, f16 ? 64 : 32), Cp = round_up(Cout, 256);
    const char *ea = HMV_DEV_ENV("HMV_BENCH_APAD"), *ew = HMV_DEV_ENV("HMV_BENCH_WPAD");
    const int lda = Cin + (ea ? atoi(ea) : 0), ldw = Kpad + (ew ? atoi(ew) : 0);
    const size_t nin = (size_t)N * H * W * lda, nout = (size_t)N * Ho * Wo * Cout, nw = (size_t)Cp * ldw;
    float *din = nullptr, *dout = nullptr, *dw = nullptr, *db = nullptr, *dres = nullptr;
    const char *esk = HMV_DEV_ENV("HMV_BENCH_SKEW");   // bytes by which the output buffer is displaced inside its allocation
    const size_t skew = esk ? (size_t)atol(esk) : 0;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&din), nin * eb);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&dout), nout * eb + skew);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&dw), nw * eb);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&db), (size_t)Cp * 4);
    if (e == hipSuccess && with_residual) e = hipMalloc(reinterpret_cast<void **>(&dres), nout * eb);
    if (e == hipSuccess) {
        // pseudo-random (not zero: zero operands raise the clock and flatter the number)
        const size_t nmax = std::max(std::max(nin, nw), with_residual ? nout : (size_t)1);
        std::vector<float> hbuf(f16 ? 0 : nmax);
        std::vector<_Float16> hh(f16 ? nmax : 0);
        uint32_t st = 12345u;
        auto fill = [&](float *d, size_t n) {
            for (size_t i = 0; i < n; ++i) {
                st = st * 1664525u + 1013904223u;
                const float v = ((st >> 8) * (1.0f / 8388608.0f)) - 1.0f;
                if (f16) hh[i] = (_Float16)v; else hbuf[i] = v;
            }
            return hipMemcpy(d, f16 ? (const void *)hh.data() : (const void *)hbuf.data(), n * eb, hipMemcpyHostToDevice);
        };
        e = fill(din, nin);
        if (e == hipSuccess) e = fill(dw, nw);
        if (e == hipSuccess && with_residual) e = fill(dres, nout);
        if (e == hipSuccess) e = hipMemset(db, 0, (size_t)Cp * 4);
    }
    if (e == hipSuccess) {
        ConvParams p{};
        p.in = din; p.wgt = dw; p.bias = db; p.res = dres; p.out = reinterpret_cast<char *>(dout) + skew;
        p.in_f16 = f16; p.out_f16 = f16; p.res_f16 = f16 && dres;
        p.N = N; p.H = H; p.W = W; p.Cin = Cin; p.Ho = Ho; p.Wo = Wo; p.Cout = Cout;
        p.R = R; p.S = S; p.stride = stride; p.pad_h = pad; p.pad_w = pad; p.K = K; p.Kpad = Kpad;
        p.M = N * Ho * Wo; p.ldc = Cout; p.ldr = Cout; p.act = ACT_RELU; p.osy = p.osx = 1;
        p.lda = lda; p.ldw = ldw;
        p.tall = HMV_DEV_ENV("HMV_BENCH_TALL") != nullptr;   // the tall-tile 3x3 kernel (conv_ht.hip); random weights have no order
        unsigned long long *ddbg = nullptr;
        const int nblk_dbg = ((p.M + 63) / 64) * ((Cout + 31) / 32);
        if (HMV_DEV_ENV("HMV_BENCH_CLOCK")) {
            (void)hipMalloc(reinterpret_cast<void **>(&ddbg), (size_t)nblk_dbg * 64);
            (void)hipMemset(ddbg, 0, (size_t)nblk_dbg * 64);
            p.dbg = ddbg;
        }
        const ConvTile t = tile < 0 ? conv_pick_tile(p.M, Cout, K, f16, dres != nullptr) : (ConvTile)tile;
        hipEvent_t e0, e1;
        (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
        for (int i = 0; i < 2 && e == hipSuccess; ++i) e = launch_conv(p, t, nullptr);
        if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
        for (int i = 0; i < iters && e == hipSuccess; ++i) e = launch_conv(p, t, nullptr);
        if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (avg_ms) *avg_ms = ms / (float)iters;
        if (ddbg) {
            std::vector<unsigned long long> hd((size_t)nblk_dbg * 8);
            (void)hipMemcpy(hd.data(), ddbg, hd.size() * 8, hipMemcpyDeviceToHost);
            if (const char *dump = HMV_DEV_ENV("HMV_BENCH_DUMP")) {
                if (FILE *f = fopen(dump, "wb")) { fwrite(hd.data(), 8, hd.size(), f); fclose(f); }
            }
            if (HMV_DEV_ENV("HMV_BENCH_PHASES"))   // conv_hs.hip: {wait, main loop, epilogue} cycles of workgroup 0's first wave, blocks, total
                fprintf(stderr, "[phases] wait %llu main %llu epilogue %llu blocks %llu total %llu\n", hd[0], hd[1], hd[2], hd[3], hd[4]);
            std::vector<double> clk, cyc;
            for (int i = 0; i < nblk_dbg; ++i)
                if (hd[8 * i + 1] > 0) { clk.push_back((double)hd[8 * i] / (double)hd[8 * i + 1] * 0.1); cyc.push_back((double)hd[8 * i]); }
            if (!clk.empty()) {
                std::sort(clk.begin(), clk.end()); std::sort(cyc.begin(), cyc.end());
                fprintf(stderr, "[clock] blocks=%zu median %.3f GHz (p10 %.3f p90 %.3f), median main-loop cycles %.0f\n", clk.size(),
                        clk[clk.size() / 2], clk[clk.size() / 10], clk[clk.size() * 9 / 10], cyc[cyc.size() / 2]);
            }
            (void)hipFree(ddbg);
        }
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    for (float *ptr : {din, dout, dw, db, dres}) if (ptr) (void)hipFree(ptr);
    if (e != hipSuccess) { g_create_err = std::string("hmv_bench_conv: ") + hipGetErrorString(e); return HMV_ERR_HIP; }
    return HMV_OK;
}

int hmv_op_conv2d_ex(int32_t device, int32_t dtype, const float *in, int32_t N, int32_t H, int32_t W, int32_t Cin,
                     const float *w_oihw, const float *bias_host, int32_t Cout, int32_t R, int32_t S, int32_t stride, int32_t pad,
                     const float *residual, int32_t relu, float *out, void *stream);
}  // extern "C"

// ====================================================================== forward
namespace {

// second A source of a conv (Bottleneck conv3 + downsample as one GEMM over [t2 | x(strided)])
struct Dual { const float *in2 = nullptr; int ksplit = 0, H2 = 0, W2 = 0, lda2 = 0, stride2 = 1; };

// An activation map in the workspace, channels-last: [N][H][W][ld] with C real channels, ld the row stride in elements
struct Map { float *p = nullptr; int N = 0, H = 0, W = 0, C = 0, ld = 0; };
inline int conv_out(int n, int k, int stride, int pad) { return (n + 2 * pad - k) / stride + 1; }   // output size of a conv along one axis

// What a backbone hands on: the n sampled feature levels in the reference's feats[] order (handmvnet.py:165-177) and the heat-map logits
// (fp32, row stride 32)
struct Features { Map lv[4]; int n = 0; Map hm; };

// One conv / GEMM launch of a packed Layer, said whole: what is not named at the call site has its default here
struct ConvCall {
    const Layer *L;
    const float *in; int N, H, W;             // NHWC [N][H][W][L.Cin]
    float *out; int ldc, Ho, Wo;
    int stride = 1, pad_h = 0, pad_w = 0;
    const float *res = nullptr; int ldr = 0;
    int activation = ACT_NONE;
    bool out_f16 = false, fill = false;
    int up = 0;
    int rg_out = 0, rg_in = 0;                // residual row remap
    int scatter = 0, ooy = 0, oox = 0;        // transposed-conv phase placement
    int ksplit = 1;                           // split-K slices
    int phases = 0; size_t phase_stride = 0;  // 4: the four transposed-conv phases in one launch (weights phase_stride apart)
    Dual dual;
    const Layer *next = nullptr; float *next_out = nullptr;   // chained 1x1 conv + ReLU (conv_stream.hip)
    int pool_h = 0, pool_w = 0;               // MaxPool2d(3, 2, 1) fused behind it (conv_hs.hip, the fp16 stem): `out` is then the pooled map
    bool mapped = false, maps_ok = true;      // built from two Maps: Runner::conv holds the output map to the conv's own output grid

    // a launch whose output buffer is not the conv's own output grid: GEMM rows (N = rows, H = W = 1), transposed-conv phases, the pooled
    // stem, an up-sampling fuse term, the op-level entries
    ConvCall(const Layer &L_, const float *in_, int N_, int H_, int W_, float *out_, int ldc_, int Ho_, int Wo_)
        : L(&L_), in(in_), N(N_), H(H_), W(W_), out(out_), ldc(ldc_), Ho(Ho_), Wo(Wo_) {}
    ConvCall(const Layer &L_, const Map &x, const Map &y)
        : L(&L_), in(x.p), N(x.N), H(x.H), W(x.W), out(y.p), ldc(y.ld), Ho(y.H), Wo(y.W), mapped(true),
          maps_ok(x.N == y.N && x.ld >= x.C && y.ld >= y.C) {}
    ConvCall &s(int v) { stride = v; return *this; }
    ConvCall &pad(int ph, int pw) { pad_h = ph; pad_w = pw; return *this; }
    ConvCall &pad(int v) { return pad(v, v); }   // both ways
    ConvCall &add(const float *r, int ld) { res = r; ldr = ld; return *this; }
    ConvCall &res_rows(int out_group, int in_group) { rg_out = out_group; rg_in = in_group; return *this; }
    ConvCall &act(int a) { activation = a; return *this; }
    ConvCall &f16(bool v) { out_f16 = v; return *this; }
    ConvCall &filled(bool v = true) { fill = v; return *this; }
    ConvCall &upsample(int shift) { up = shift; return *this; }
    ConvCall &phase(int oy, int ox) { scatter = 1; ooy = oy; oox = ox; return *this; }
    ConvCall &all_phases(int n, size_t wstride) { scatter = 1; phases = n; phase_stride = wstride; return *this; }
    ConvCall &split_k(int slices) { ksplit = slices; return *this; }
    ConvCall &second(const float *x, int k0, int Hx, int Wx, int ldx, int sx) { dual = Dual{x, k0, Hx, Wx, ldx, sx}; return *this; }
    ConvCall &chain(const Layer &nx, float *nx_out) { next = &nx; next_out = nx_out; return *this; }
    ConvCall &pooled(int ph, int pw) { pool_h = ph; pool_w = pw; return *this; }
};

// One forward in progress: workspace, stream and launch helpers, the two residual blocks, then the stages of HandMvNet.forward
// A ragged call's view sets: N frames in all, sample b's token rows are seg[b] .. seg[b + 1] (device, B + 1 entries), frame n sits at
// positions fpos[n] .. fpos[n] + 20 of its sample (device, N entries); Tmax = the longest sample's token count.  A planning run has no tables.
struct ViewSet { int N; const int32_t *seg, *fpos; int Tmax; };

// Raw camera frames instead of a prepared NCHW input (hmv_forward_frames*); frames == nullptr: the call brings x
struct FrameSrc {
    const uint8_t *frames = nullptr;
    const int *boxes = nullptr;
    const int *index = nullptr;   // hmv_forward_frames_views: packed frame n is frames / boxes [index[n]] of the caller's n_src
    int n_src = 0;
    int fh = 0, fw = 0;
    float mean[3] = {0, 0, 0}, std[3] = {1, 1, 1};
    const int *rects = nullptr;   // hmv_forward_frames_occlusions: packed frame n's occluder, window pixels (device, [n][4])
};
// The tracking tail (hmv_forward_frames_track / hmv_forward_frames_views_track): behind the forward, on its stream, the windows
// (src.boxes) and bbox are moved in place to the box around the joints just found (track.hip)
struct TrackTail { bool on = false; int margin = 0, square = 1; float *joints_img = nullptr; int *status = nullptr; };
// One forward call, whole: built by the public entry from its arguments and passed down by const reference; the handle keeps nothing of
// it.  A planning run is the call with nothing but its batch
struct ForwardCall {
    int batch = 0;
    const float *x = nullptr;   // prepared NCHW input, or ...
    FrameSrc src;               // ... raw frames
    const float *bbox = nullptr, *intrinsic = nullptr;
    float *joints_crop_img = nullptr, *joints_cam = nullptr, *heatmap = nullptr;
    TrackTail track;
    hipStream_t stream = nullptr;
};

#define LAUNCH(expr) launch(#expr, [&] { return (expr); })   // (inside Runner: see launch())
struct Runner {
    hmv_engine *h;
    hipStream_t s;
    bool dry;
    int rc = HMV_OK;
    Arena &A;
    const ViewSet *vs = nullptr;   // not null: a ragged forward (hmv_forward_views); stages are not captured then
    bool sweep = false;            // a camera-subset sweep (hmv_forward_subsets): the token rows leave tokens_stage without PE and pair copy; no stages
    const FrameSrc *src = nullptr;   // the call's frame source (null in the op-level entries): the backbones prepare their input from it
    float *tokens_dst = nullptr;     // an occlusion sweep: tokens_stage writes its rows here (the caller's, kept) instead of rows of its own

    float *alloc(size_t n) {
        float *ptr = A.alloc(n);
        // a real run must stay inside the reservation its planning run sized: stop launching before anything touches memory past it
        if (!dry && h->arena_bytes && A.high > h->arena_bytes && rc == HMV_OK) rc = h->fail(HMV_ERR_STATE, "workspace plan exceeded its reservation");
        return ptr;
    }
    // Two streams (HRNet: a module's last branch beside the one above it): nothing freed inside the region may be handed out again before
    // the streams have joined -- its last user may still be running on the other stream -- so releases wait in `deferred` until join().
    // Same alloc / release sequence in the planning run.
    bool defer = false;
    std::vector<float *> deferred;
    void release(float *p) {
        if (defer && p) deferred.push_back(p);
        else A.release(p);
    }
    // fp16 path: the conv stack (stem .. pose_net / sample convs) stores activations as fp16; heat-map logits,
    // coordinates, tokens, fusion and decoder stay fp32.  ACT(n) = arena floats for n activation elements.
    const bool h16 = h->cfg.dtype != HMV_F32;      // the conv stack runs on the fp16 kernels ...
    const bool split = h->cfg.dtype == HMV_F32X3;  // ... on (hi, lo) pairs: 4 bytes per element like fp32
    size_t ACT(size_t n) const { return (h16 && !split) ? (n + 1) / 2 : n; }
    // A map's allocation is sized by its own dims: a conv-stack activation (ld = 0: the NHWC channel stride cpad(C)), or fp32 whatever the mode
    Map act(int N, int H, int W, int C, int ld = 0) {
        Map m{nullptr, N, H, W, C, ld ? ld : cpad(C)};
        m.p = alloc(ACT((size_t)N * H * W * m.ld));
        return m;
    }
    Map f32map(int N, int H, int W, int C, int ld) { return Map{alloc((size_t)N * H * W * ld), N, H, W, C, ld}; }
    void release(const Map &m) { release(m.p); }
    void fork() {   // the second stream starts behind everything enqueued so far
        defer = true;
        if (dry || rc != HMV_OK) return;
        check(hipEventRecord(h->ev_fork, s), "hipEventRecord");
        check(hipStreamWaitEvent(h->aux, h->ev_fork, 0), "hipStreamWaitEvent");
    }
    void join() {   // ... and the first one continues behind everything the second has enqueued
        if (!dry && rc == HMV_OK) {
            check(hipEventRecord(h->ev_join, h->aux), "hipEventRecord");
            check(hipStreamWaitEvent(s, h->ev_join, 0), "hipStreamWaitEvent");
        }
        defer = false;
        for (float *p : deferred) A.release(p);
        deferred.clear();
    }

    void check(hipError_t e, const char *what) {
        if (e != hipSuccess && rc == HMV_OK) rc = h->fail(HMV_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    }

    // every launch that is not a conv: `f` is not evaluated in a planning run or after an error; n = launches behind the one call
    template <class F> void launch(const char *what, F &&f, int n = 1) {
        if (!dry && rc == HMV_OK) { check(f(), what); h->launches += n; }
    }

    // Fusion block l's attention map, directly behind its attention launch, where hmv_set_attention_capture selected the block (a sweep
    // ignores the mask).  kind / q / k / pr as launch_attention_probs takes them; views > 0: the block's keys are whole views, the share per
    // view follows (rank0: the view rank of key 0).  A ragged call's map is zero-filled first; a block without keys (one view in the
    // cross block) launches nothing on an empty grid and leaves a share of zeros.
    void attention_map(int l, int kind, const void *q, int q_ld, const void *k, int kv_ld, int B, const AttnProbsRows &pr, int rank0, int views) {
        if (dry || sweep || !((h->att_mask >> l) & 1u) || rc != HMV_OK) return;
        hmv_engine::AttMap &m = h->att[l];
        const size_t n = (size_t)B * 8 * pr.Tq_pad * pr.Tk_pad, ns = (size_t)B * 8 * pr.Tq_pad * views;
        if (n > m.probs_cap || ns > m.share_cap) {
            rc = h->fail(HMV_ERR_STATE, "attention map of block %d exceeds its buffers", l);
            return;
        }
        if (pr.seg && n) LAUNCH(hipMemsetAsync(m.probs, 0, n * sizeof(float), s));
        if (n) LAUNCH(launch_attention_probs(kind, q, q_ld, k, kv_ld, B, pr, m.probs, s));
        if (ns && n) LAUNCH(launch_attention_share(m.probs, B, pr, rank0, views, m.share, s));
        else if (ns) LAUNCH(hipMemsetAsync(m.share, 0, ns * sizeof(float), s));
        m.valid = rc == HMV_OK;
        m.B = B; m.Tq = pr.Tq_pad; m.Tk = pr.Tk_pad; m.views = views;
    }

    const char **kernel_name = nullptr;   // op-level entries: receives the kernel family of the last launch
    ConvRoute route = conv_rule();        // the kernel families its launches may take (op-level entries: from a kernel_sel); planning asks with it too

    // The launch `c` describes, as the launchers see it.  Pure: no launch, no allocation, no state -- the planning run asks the same
    // questions of it (chains_into(), the pooled stem) as the real one
    ConvParams params(const ConvCall &c) const {
        const Layer &L = *c.L;
        ConvParams p{};
        p.in = c.in; p.wgt = L.w; p.bias = L.bias; p.res = c.res; p.out = c.out;
        if (c.ksplit > 1) { p.ksl = c.ksplit; p.kslice = L.Kpad / c.ksplit; p.out_slice = (size_t)c.N * c.Ho * c.Wo * c.ldc; }
        if (c.phases > 1) { p.phases = c.phases; p.phase_stride = c.phase_stride; }
        if (c.dual.in2) {
            p.in2 = c.dual.in2; p.ksplit = c.dual.ksplit; p.H2 = c.dual.H2; p.W2 = c.dual.W2; p.lda2 = c.dual.lda2; p.stride2 = c.dual.stride2;
            p.lda = c.dual.ksplit;   // the first source's pixel stride is its own channel count, not the concatenated one
        }
        p.in_f16 = L.f16; p.out_f16 = c.out_f16; p.res_f16 = L.f16 && c.res != nullptr;   // a residual always has the layer's dtype
        p.N = c.N; p.H = c.H; p.W = c.W; p.Cin = L.Cin;
        p.Ho = c.Ho; p.Wo = c.Wo; p.Cout = L.Cout;
        p.R = L.R; p.S = L.S; p.stride = c.stride; p.pad_h = c.pad_h; p.pad_w = c.pad_w;
        p.K = L.K; p.Kpad = L.Kpad;
        p.M = c.N * c.Ho * c.Wo;
        p.ldc = c.ldc; p.ldr = c.ldr; p.act = c.activation;
        p.rg_out = c.rg_out; p.rg_in = c.rg_in;
        p.scatter = c.scatter; p.osy = c.scatter ? 2 : 1; p.osx = c.scatter ? 2 : 1; p.ooy = c.ooy; p.oox = c.oox;
        p.up = c.up; p.fill = c.fill ? 1 : 0;
        p.tall = L.tall;
        if (L.rd_cout) { p.rd_cout = L.rd_cout; p.pad_w = 0; }   // L.R x L.S is the 3x1 GEMM, the epilogue sums the s groups
        if (L.plane) {   // HMV_F32X3: [hi | lo] rows in, pairs out (unless this layer writes fp32), pairs as residual
            p.lda = 2 * L.plane;
            if (L.x3n) p.x3_plane = L.plane;
            else p.cwrap = 2 * L.plane;
            p.acc_shift = L.acc_shift;
            if (c.out_f16) { p.out_split = 1; p.ldc = 2 * c.ldc; p.sat = h->sat; }
            if (c.res) { p.res_split = 1; p.ldr = 2 * c.ldr; }
        }
        if (c.pool_h > 0) { p.pool = 1; p.pool_h = c.pool_h; p.pool_w = c.pool_w; }
        if (const Layer *Lx = c.next) {
            p.nx_wgt = Lx->w; p.nx_bias = Lx->bias; p.nx_out = c.next_out; p.nx_cout = Lx->Cout; p.nx_ldw = Lx->Kpad; p.nx_ldc = Lx->Cout;
            p.nx_act = ACT_RELU;
        }
        return p;
    }

    // Would the conv3 launch `c3` also compute conv1 + BN + ReLU of the block behind it (conv_stream.hip "chain")?  That block's conv1
    // reads this launch's output and nothing else, so a workgroup that holds all channels of its pixels computes it from the tile in
    // LDS (fp16 layer1 at large batches: the 256-channel tensor is read once less per block).  Bit-identical to the two launches, so
    // the answer may depend on the launch size (conv_stream_chain_ok).  `c3` as it would launch WITHOUT the chain
    bool chains_into(const ConvCall &c3, const Block *nb) const {
        if (!h->chain_fuse || !nb || h->cfg.dtype != HMV_F16) return false;
        const Layer &n1 = nb->c1;
        const int outc = c3.L->Cout;
        return n1.f16 && !n1.plane && n1.R == 1 && n1.S == 1 && n1.Cin == outc && n1.K == outc && n1.Kpad == outc && !n1.tall && !n1.rd_cout &&
               conv_stream_chain_ok(params(c3), n1.Cout, route);
    }

    // One profiled launch: take a record (its events are made once and reused), stamp e0; the caller fills flops and bytes
    ProfRec *prof_begin(std::string label) {
        if (h->prof_used == h->prof.size()) {
            ProfRec r{};
            check(hipEventCreate(&r.e0), "hipEventCreate");
            check(hipEventCreate(&r.e1), "hipEventCreate");
            h->prof.push_back(r);
        }
        ProfRec *pr = &h->prof[h->prof_used++];
        pr->label = std::move(label);
        check(hipEventRecord(pr->e0, s), "hipEventRecord");
        return pr;
    }
    void prof_end(ProfRec *pr, const char *kernel) {
        if (pr) { pr->name = kernel; check(hipEventRecord(pr->e1, s), "hipEventRecord"); }
    }

    // Algorithmic cost of one conv launch (what bench.py's roofline divides by).  FLOPs: the real (un-padded) reduction length -- the
    // stem's 4th channel is padding.  Bytes: each input pixel the window touches once, the weights once, residual and output rows once;
    // a (hi, lo) pair is 4 bytes like fp32; a strided 1x1 conv reads only the pixels it keeps.  (FLOPs count L.Cout, bytes the real
    // output channels of a row-decomposed layer.)  pooled, dual and phases never meet in one launch; if they did, the first in that
    // order would decide the bytes
    static void conv_cost(const ConvCall &c, const ConvParams &p, double &flops, double &bytes) {
        const Layer &L = *c.L;
        const double kreal = L.Kreal ? (double)L.Kreal : (double)L.K;   // real channels only (no padding FLOPs)
        const double cout_real = L.rd_cout ? (double)L.rd_cout : (double)L.Cout;
        const double eb_in = L.f16 ? (L.plane ? 4.0 : 2.0) : 4.0;
        const double eb_out = (L.f16 && c.out_f16) ? (L.plane ? 4.0 : 2.0) : 4.0;
        const double cin_real = L.in_real ? (double)L.in_real : kreal / (double)(L.R * L.S);   // (the row-decomposed form has R x S = 3 x 1 and Kreal = 3 * Cin)
        const bool pointwise = L.R == 1 && L.S == 1;
        const double in_px = (pointwise && c.stride > 1) ? (double)p.M : (double)c.N * c.H * c.W;
        const double in_b = in_px * cin_real * eb_in, w_b = (double)L.Cout * kreal * eb_in, out_b = (double)p.M * cout_real * eb_out;
        flops = 2.0 * (double)p.M * (double)L.Cout * kreal;
        if (c.phases > 1) flops *= c.phases;
        if (p.pool)   // the conv map never reaches HBM: input, weights, the pooled map
            bytes = in_b + w_b + (double)c.N * p.pool_h * p.pool_w * cout_real * eb_out;
        else if (c.dual.in2)   // [t2 | x]: t2 at every output pixel, x at the pixels the stride keeps
            bytes = ((double)p.M * c.dual.ksplit + (double)p.M * (kreal - c.dual.ksplit)) * eb_in + w_b + out_b;
        else if (c.phases > 1)   // every phase: its own weights and output pixels, the same input
            bytes = in_b + c.phases * (w_b + out_b);
        else
            bytes = in_b + w_b + out_b + (c.res ? (double)p.M * cout_real * eb_in : 0.0);
        if (const Layer *Lx = c.next) {   // the chained conv: its weights and output rows; its input rows never leave the CU
            flops += 2.0 * (double)p.M * (double)Lx->Cout * (double)Lx->K;
            bytes += (double)Lx->Cout * (double)Lx->K * eb_in + (double)p.M * (double)Lx->Cout * eb_out;
        }
    }

    // One conv / GEMM launch
    void conv(const ConvCall &c) {
        if (dry || rc != HMV_OK) return;
        const Layer &L = *c.L;
        // two Maps: the output map is the grid the input map, R x S, stride and pad imply (a row-decomposed 3x3 is packed as 3x1), no row
        // stride cuts its channels -- else stop, like alloc(), before anything is launched
        if (c.mapped && !(c.maps_ok && c.Ho == conv_out(c.H, L.R, c.stride, c.pad_h) && c.Wo == conv_out(c.W, L.rd_cout ? L.R : L.S, c.stride, c.pad_w))) {
            rc = h->fail(HMV_ERR_STATE, "%s: output map %d x %d does not fit its input %d x %d", L.label.c_str(), c.Ho, c.Wo, c.H, c.W);
            return;
        }
        const ConvParams p = params(c);
        // split layers walk 3x the reduction on fp16 MFMAs: the tile rules see the real reduction length
        const ConvTile tile = conv_pick_tile(p.M, p.Cout, L.plane ? p.K / (L.x3n ? 2 : 3) : p.K, L.f16, c.res != nullptr);
        ProfRec *pr = nullptr;
        if (h->profiling) {
            pr = prof_begin(c.next ? L.label + "+" + c.next->label : (p.pool ? L.label + "+maxpool" : L.label));
            conv_cost(c, p, pr->flops, pr->bytes);
        }
        const char *kname = nullptr;
        check(launch_conv(p, tile, s, &kname, route), L.label.c_str());
        ++h->launches;
        if (kernel_name) *kernel_name = kname;
        prof_end(pr, kname);
    }

    // the up-sampling terms of an HRNet fuse layer in one launch (hr_fuse.hip)
    void hr_fuse_up(const HrFuseParams &p, const std::string &label) {
        if (dry || rc != HMV_OK) return;
        ProfRec *pr = nullptr;
        if (h->profiling) {
            pr = prof_begin(label);
            const double eb = p.f16 ? 2.0 : 4.0;
            pr->flops = 0.0;
            pr->bytes = 2.0 * (double)p.N * p.H * p.W * p.C * eb;   // the map once in, once out
            for (int q = 0; q < p.nsrc; ++q) {   // the products at the sources' own resolution
                const HrFuseSrc &S = p.src[q];
                pr->flops += 2.0 * (double)p.N * S.H * S.W * S.C * p.C;
                pr->bytes += (double)p.N * S.H * S.W * S.C * eb + (double)S.C * p.C * 4.0;
            }
        }
        check(launch_hr_fuse_up(p, s), label.c_str());
        ++h->launches;
        prof_end(pr, p.f16 ? "hr_fuse_up_f16" : "hr_fuse_up_f32");
    }

    static int splitk_slices(const Layer &L, int rows) {
        static const bool no_splitk = HMV_DEV_ENV("HMV_NO_SPLITK") != nullptr;   // development knob (A/B runs)
        return (!no_splitk && !L.f16 && L.R == 1 && L.S == 1 && !L.plane && L.Kpad >= 1024 && L.Kpad % 128 == 0 &&
                L.Cout <= 4096 /* zero_bias */ && rows > 0) ? 4 : 1;
    }
    // the S partial products a . W of the K slices, one launch, [S][rows][lds] into `slab`; whoever sums them adds L's bias
    void conv_slices(const Layer &L, const float *a, int rows, int S, float *slab, int lds) {
        Layer Ls = L;
        Ls.bias = h->zero_bias;
        conv(ConvCall(Ls, a, rows, 1, 1, slab, lds, 1, 1).split_k(S));
    }

    // y = LayerNorm(...) tail of a split-K GEMM (gemm_ln below)
    struct LnTail { const float *g1, *b1, *g2, *b2; float *y, *y2; int ldy; };

    // split-K (layers.py:224 to_out: K = 1024, and 2048 in the learnable-query blocks): a long reduction over few token rows
    // tiles into a few dozen workgroups at a small batch.  K is cut into 4 slices that run as 4x the workgroups of ONE
    // launch; a reduction kernel adds the partial products in slice order and applies bias / residual / activation -- or, when the
    // consumer is a LayerNorm (`ln`), slice sum, bias and residual become that kernel's load.
    // The cut depends on K alone -- never on the batch -- so a sample's result does not depend on what it is batched with
    // (tests/test_gpu_parity.py::test_full_size_properties).  Same alloc / release sequence in the dry (planning) run.
    void gemm_splitk(const Layer &L, const float *a, int rows, float *out, int ldc, const float *res, int ldr, int act, int rg_out, int rg_in,
                     const LnTail *ln) {
        const int S = splitk_slices(L, rows), lds_ = (L.Cout + 3) / 4 * 4;
        float *slab = alloc((size_t)S * rows * lds_);
        conv_slices(L, a, rows, S, slab, lds_);
        if (ln)
            launch("splitk_layernorm", [&] { return launch_splitk_layernorm(slab, S, rows, lds_, L.Cout, L.bias, res, ldr, rg_out, rg_in, ln->g1, ln->b1,
                                                                            ln->y, ln->ldy, ln->g2, ln->b2, ln->y2, s); });
        else
            launch("splitk_reduce", [&] { return launch_splitk_reduce(slab, S, rows, lds_, L.Cout, L.bias, res, ldr, rg_out, rg_in, act, out, ldc, s); });
        release(slab);
    }

    void gemm(const Layer &L, const float *a, int rows, float *out, int ldc, const float *res, int ldr, int act, int rg_out = 0,
              int rg_in = 0) {
        if (splitk_slices(L, rows) > 1) gemm_splitk(L, a, rows, out, ldc, res, ldr, act, rg_out, rg_in, nullptr);
        else conv(ConvCall(L, a, rows, 1, 1, out, ldc, 1, 1).add(res, ldr).act(act).res_rows(rg_out, rg_in));
    }

    // Everything of a fusion block behind the attention in two launches: the split-K to_out GEMM, then ONE kernel for
    // (slice sum + bias + residual) -> [LayerNorm1] -> FeedForward (LayerNorm, Linear, GELU, Linear, + residual) -> [LayerNorm2]
    // (fusion_kernels.hip).  Same alloc / release sequence in the dry (planning) run.
    bool ff_fusable(const AttnLayer &a, int rows, bool have_x3 = false) const {
        const Layer &ff1 = a.ff1, &ff2 = a.ff2;
        const int ldt = h->ldt;
        return h->ff_fuse && (have_x3 || splitk_slices(a.out, rows) > 1) && !ff1.f16 && !ff2.f16 && !ff1.plane && !ff2.plane &&
               ff1.Kpad == ldt && ldt % 16 == 0 && (ff1.Cout == 128 || ff1.Cout == 256) && ff2.Kpad == ff1.Cout && ff2.Cout_pad >= ldt &&
               ldt <= 576;
    }
    // The layers, the LayerNorm vectors (null where the block has none) and the split-pair to_out are `a`'s; rows of `att` in, token rows
    // `y` (and their (hi, lo) pair copy `y_pairs`, if not null) out, both with row stride ldt like the residual rows `res`
    void ff_block(const AttnLayer &a, const float *att, int rows, const float *res, int rg_out, int rg_in, float *y, float *y_pairs, bool x3) {
        const Layer &out = a.out, &ff1 = a.ff1, &ff2 = a.ff2;
        const int ldt = h->ldt;
        // x3: `att` holds (hi, lo) pairs and to_out runs as ONE split-pair GEMM (gemm_x3.hip) instead of four fp32 split-K slices
        const int S = x3 ? 1 : splitk_slices(out, rows), lds_ = (out.Cout + 3) / 4 * 4;
        float *slab = alloc((size_t)S * rows * lds_);
        if (x3) conv(ConvCall(a.out_x3, att, rows, 1, 1, slab, lds_, 1, 1));   // (its own bias is zero)
        else conv_slices(out, att, rows, S, slab, lds_);
        launch("ff_block", [&] {
            FfBlockParams p{};
            p.slab = slab; p.S = S; p.slice = (size_t)rows * lds_; p.lds = lds_; p.bias0 = out.bias;
            p.res = res; p.ldr = ldt; p.rg_out = rg_out; p.rg_in = rg_in;
            p.rows = rows; p.d = h->d; p.ld = ldt;
            p.n1g = a.n1g; p.n1b = a.n1b; p.fg = a.fg; p.fb = a.fb; p.n2g = a.n2g; p.n2b = a.n2b;
            p.w1 = ff1.w; p.b1 = ff1.bias; p.ldw1 = ff1.Kpad; p.w2 = ff2.w; p.b2 = ff2.bias; p.ldw2 = ff2.Kpad;
            p.out = y; p.ldo = ldt; p.hid = ff1.Cout; p.out_pairs = y_pairs; p.sat = h->sat;
#ifdef HMV_DEV_KNOBS
            static unsigned long long *ffdbg = nullptr;   // HMV_FF_DBG=1: phase stamps of the last launch, printed by the next one (never under graph capture)
            if (HMV_DEV_ENV("HMV_FF_DBG")) {
                if (!ffdbg) (void)hipMalloc(reinterpret_cast<void **>(&ffdbg), 4096 * 64);
                else {
                    unsigned long long hst[8 * 4];
                    (void)hipStreamSynchronize(s);
                    (void)hipMemcpy(hst, ffdbg, sizeof(hst), hipMemcpyDeviceToHost);
                    for (int w = 0; w < 2; ++w)
                        fprintf(stderr, "[ff_block wg %d] phase0 %.2f us  gemm1 %.2f  gemm2 %.2f  ln2+store %.2f  (entry->exit %.2f us)\n", w * 3,
                                (hst[w * 24 + 1] - hst[w * 24]) * 0.01, (hst[w * 24 + 2] - hst[w * 24 + 1]) * 0.01, (hst[w * 24 + 3] - hst[w * 24 + 2]) * 0.01,
                                (hst[w * 24 + 4] - hst[w * 24 + 3]) * 0.01, (hst[w * 24 + 4] - hst[w * 24]) * 0.01);
                }
                p.dbg = ffdbg;
            }
#endif
            return launch_ff_block(p, s);
        });
        release(slab);
    }

    // y = LayerNorm(a . W + bias + residual) (+ a chained second LayerNorm y2): layers.py:224-229 (to_out, + _q, norm1, then the
    // FeedForward's own LayerNorm).  With split-K the GEMM's reduction kernel IS the LayerNorm kernel (one launch less per block).
    void gemm_ln(const Layer &L, const float *a, int rows, const float *res, int ldr, int rg_out, int rg_in, const float *g1,
                 const float *b1, float *y, int ldy, const float *g2, const float *b2, float *y2) {
        if (splitk_slices(L, rows) > 1) {
            const LnTail ln{g1, b1, g2, b2, y, y2, ldy};
            gemm_splitk(L, a, rows, nullptr, 0, res, ldr, ACT_NONE, rg_out, rg_in, &ln);
            return;
        }
        float *o = alloc((size_t)rows * ldy);
        gemm(L, a, rows, o, ldy, res, ldr, ACT_NONE, rg_out, rg_in);
        launch("layernorm", [&] { return launch_layernorm(o, ldy, rows, L.Cout, g1, b1, y, ldy, g2, b2, y2, s); });
        release(o);
    }

    // q/k/v projection of fp32 token rows; in the fp16 / f32x3 modes on the fused split kernels (Loader::linear_x3)
    // pairs_out: the result rows as (hi, lo) fp16 pairs [hi ldc | lo ldc] (the GEMM's pair epilogue; same bytes as fp32 rows) for a consumer
    // that multiplies on the fp16 matrix cores (attention_x3_kernel)
    void project(const Layer &L, const float *a, int rows, float *out, int ldc, float *ready_pairs = nullptr, bool pairs_out = false) {
        if (!L.plane) { gemm(L, a, rows, out, ldc, nullptr, 0, ACT_NONE); return; }
        float *pairs = ready_pairs;
        if (!pairs) {
            pairs = alloc((size_t)rows * h->ldt);                           // [hi ldt | lo ldt] halfs per row
            launch("rows_f32_to_half", [&] { return launch_rows_f32_to_half(a, pairs, (size_t)rows, h->ldt, 2, s, h->sat); });
        }
        conv(ConvCall(L, pairs, rows, 1, 1, out, ldc, 1, 1).f16(pairs_out));
        release(pairs);
    }

    // Bottleneck (resnet.py:124-144; HRNet's layer1): -> its output map; the caller releases `x`.  `t1`: conv1 + BN + ReLU of this block
    // where the previous block's chained conv3 launch computed it (conv_stream.hip chain), else no map; on return the same for the block
    // behind this one, `nb`, whose conv1 may ride on this block's conv3 launch
    Map bottleneck(const Block &b, const Map &x, const Block *nb, Map &t1_chained) {
        const int planes = b.c1.Cout, outc = b.c3.Cout;
        const int ho = conv_out(x.H, 3, b.stride, 1), wo = conv_out(x.W, 3, b.stride, 1);
        Map t1 = t1_chained;
        if (!t1.p) {
            t1 = act(x.N, x.H, x.W, planes);
            conv(ConvCall(b.c1, x, t1).act(ACT_RELU).f16(h16));
        }
        Map t2 = act(x.N, ho, wo, planes);
        conv(ConvCall(b.c2, t1, t2).s(b.stride).pad(1).act(ACT_RELU).f16(h16));
        release(t1);
        Map dsb;
        if (b.has_ds && !b.fused_ds) {
            dsb = act(x.N, ho, wo, outc);
            conv(ConvCall(b.ds, x, dsb).s(b.stride).f16(h16));
        }
        Map y = act(x.N, ho, wo, outc);
        // fused_ds: conv3 and the downsample branch as one GEMM over [t2 | x]
        // out = relu([t2 | x(strided)] . Wcat + b): BN3 and the downsample's BN are in Wcat and b
        ConvCall c3 = b.fused_ds ? ConvCall(b.c3ds, t2, y).second(x.p, planes, x.H, x.W, x.ld, b.stride) : ConvCall(b.c3, t2, y).add(b.has_ds ? dsb.p : x.p, outc);
        c3.act(ACT_RELU).f16(h16);
        // where chains_into() says so, the conv3 launch also computes conv1 of the block behind it: into a map allocated behind this block's
        // own output, as the planning run does
        t1_chained = Map();
        if (chains_into(c3, nb)) { t1_chained = act(x.N, ho, wo, nb->c1.Cout); c3.chain(nb->c1, t1_chained.p); }
        conv(c3);
        release(t2);
        release(dsb);
        return y;
    }

    // BasicBlock (resnet.py:90-106; the branches of an HRNet module): -> its output map; the caller releases `x`.  ds: the downsample
    // conv, or null.  fill: conv1 and conv2 also write the zero pad channels of their maps (channel counts that are no multiple of 4)
    Map basic_block(const Layer &c1, const Layer &c2, const Layer *ds, int stride, const Map &x, bool fill) {
        const int outc = c1.rd_cout ? c1.rd_cout : c1.Cout;
        Map t1 = act(x.N, conv_out(x.H, 3, stride, 1), conv_out(x.W, 3, stride, 1), outc);
        conv(ConvCall(c1, x, t1).s(stride).pad(1).act(ACT_RELU).f16(h16).filled(fill));
        Map dsb;
        if (ds) {
            dsb = act(x.N, t1.H, t1.W, outc);
            conv(ConvCall(*ds, x, dsb).s(stride).f16(h16));
        }
        Map y = act(x.N, t1.H, t1.W, outc);
        conv(ConvCall(c2, t1, y).pad(1).add(ds ? dsb.p : x.p, y.ld).act(ACT_RELU).f16(h16).filled(fill));
        release(t1);
        release(dsb);
        return y;
    }

    // The first n of a chain of stride-2 3x3 convs (+ BN + ReLU) from `src` on, each into a map of its own: -> the last one (n = 0: no map)
    Map down_chain(const std::vector<Layer> &ls, size_t n, Map src) {
        Map tmp;
        for (size_t q = 0; q < n; ++q) {
            Map o = act(src.N, conv_out(src.H, 3, 2, 1), conv_out(src.W, 3, 2, 1), ls[q].Cout);
            conv(ConvCall(ls[q], src, o).s(2).pad(1).act(ACT_RELU).f16(h16).filled());
            release(tmp);
            tmp = src = o;
        }
        return tmp;
    }

    // feats[0] as fp32 NCHW into the capture buffer
    void capture_feat0(const Map &f) {
        if (!h->capture || dry || vs || sweep || !h->cap_feat0) return;
        if (split) LAUNCH(launch_nhwc_split_to_nchw(f.p, h->cap_feat0, f.N, f.H, f.W, f.C, s));
        else if (h16) LAUNCH(launch_nhwc_f16_to_nchw(f.p, h->cap_feat0, f.N, f.H, f.W, f.C, s));
        else LAUNCH(launch_nhwc_to_nchw(f.p, h->cap_feat0, f.N, f.H, f.W, f.C, s, f.ld));
    }

    // HighResolutionNet.forward (hrnet.py:357-393) and pose_net on its highest-resolution branch
    Features hrnet_backbone(int N, const float *x) {
        const HrNet &hr = h->hr;
        const int H = h->cfg.height, W = h->cfg.width;
        Map in4 = act(N, H, W, 3, h16 ? 8 : 4);   // 4 fp32 / 8 fp16 / [hi8 | lo8] per pixel
        if (src && src->frames) LAUNCH(launch_frames_to_input(src->frames, src->boxes, N, src->fh, src->fw, H, W, src->mean, src->std, split ? 2 : (h16 ? 1 : 0), in4.p, s, /*s2d=*/false, src->index, src->n_src, src->rects));
        else if (split) LAUNCH(launch_nchw_to_nhwc_split(x, in4.p, N, H, W, s, h->sat));
        else if (h16) LAUNCH(launch_nchw_to_nhwc8_f16(x, in4.p, N, H, W, s));
        else LAUNCH(launch_nchw_to_nhwc4(x, in4.p, N, H, W, s));
        Map c1 = act(N, conv_out(H, 3, 2, 1), conv_out(W, 3, 2, 1), 64);
        conv(ConvCall(hr.conv1, in4, c1).s(2).pad(1).act(ACT_RELU).f16(h16));
        release(in4);
        Map cur = act(N, conv_out(c1.H, 3, 2, 1), conv_out(c1.W, 3, 2, 1), 64);
        conv(ConvCall(hr.conv2, c1, cur).s(2).pad(1).act(ACT_RELU).f16(h16));
        release(c1);
        Map t1_chained;
        for (size_t bi = 0; bi < hr.layer1.size(); ++bi) {   // 4 Bottlenecks, planes 64 -> 256 channels
            Map y = bottleneck(hr.layer1[bi], cur, bi + 1 < hr.layer1.size() ? &hr.layer1[bi + 1] : nullptr, t1_chained);
            release(cur);
            cur = y;
        }
        Map xs[4], pre[4] = {cur};
        int npre = 1;
        for (int st = 0; st < 3; ++st) {
            const int nbr = st + 2;
            for (int i = 0; i < nbr; ++i) {   // transition layers (hrnet.py:287-311, 368-390)
                if (i >= npre) {   // a new, lower-resolution branch from the LAST previous branch
                    xs[i] = down_chain(hr.trans[st][i], hr.trans[st][i].size(), pre[npre - 1]);
                } else if (!hr.trans[st][i].empty()) {
                    xs[i] = act(N, pre[i].H, pre[i].W, hr.ch[i]);
                    conv(ConvCall(hr.trans[st][i][0], pre[i], xs[i]).pad(1).act(ACT_RELU).f16(h16).filled());
                } else {
                    xs[i] = pre[i];   // x_list.append(y_list[i]): the same tensor
                }
            }
            for (int i = 0; i < npre; ++i)
                if (xs[i].p != pre[i].p) release(pre[i]);
            for (const HrModule &M : hr.stage[st]) {   // HighResolutionModule.forward (hrnet.py:194-212)
                // Four branches: the lowest-resolution one (320 / 512 channels on 1/32-size maps: a few hundred small tiles per conv, bound
                // by request latency) runs on the second stream BESIDE the branch above it (one round of 256 x 192 tiles, latency-bound too):
                // their workgroups share the CUs.  The two highest-resolution branches own the chip with persistent kernels and stay alone.
                const bool overlap = h->hr_overlap && h16 && nbr == 4 && (dry || h->aux != nullptr);
                for (int b = 0; b < nbr; ++b) {
                    if (overlap && b == 2) fork();
                    const hipStream_t main_s = s;
                    if (overlap && b == 3) s = h->aux;
                    for (int blk = 0; blk < 4; ++blk) {
                        Map y = basic_block(M.br[b][blk][0], M.br[b][blk][1], nullptr, 1, xs[b], /*fill=*/true);
                        release(xs[b]);
                        xs[b] = y;
                    }
                    s = main_s;
                    if (overlap && b == 3) join();
                }
                // fuse: y_i = relu(sum_j f_ij(x_j)).  Every non-identity term is a conv at branch i's resolution whose
                // epilogue adds the running sum (the identity term x_i rides along as the first residual); the
                // "1x1 conv + BN + nearest upsample" terms run the 1x1 conv on the up-sampled index map instead.
                Map outs[4];
                for (int i = 0; i < nbr; ++i) {
                    const Map &xi = xs[i];
                    Map running;
                    int nterm = 0;
                    // two or more up-sampling terms (always the last of the sum): one launch for all of them (hr_fuse.hip)
                    HrFuseParams fp{};
                    bool fused = false;
                    if (h->hr_fuse && !split && nbr - 1 - i >= 2) {
                        fp.N = N; fp.H = xi.H; fp.W = xi.W; fp.C = xi.C; fp.ldc = xi.ld; fp.relu = 1; fp.f16 = h16 ? 1 : 0;
                        for (int j = i + 1; j < nbr; ++j) {
                            const Layer &l = h16 ? M.fup[i][j] : M.fuse[i][j][0];
                            HrFuseSrc &S = fp.src[fp.nsrc++];
                            S.w = l.w; S.bias = l.bias; S.C = xs[j].C; S.ld = xs[j].ld; S.ldw = l.Kpad; S.shift = j - i; S.H = xs[j].H; S.W = xs[j].W;
                        }
                        fused = fp.src[0].w != nullptr && hr_fuse_up_plan(fp);
                    }
                    for (int j = 0; j < nbr; ++j) {
                        if (j == i) continue;
                        if (fused && j > i) continue;
                        const bool first = nterm == 0, last = nterm == nbr - 2;
                        const float *res = first ? xi.p : running.p;
                        const int term_act = last ? ACT_RELU : ACT_NONE;
                        Map o = act(N, xi.H, xi.W, xi.C);
                        if (j > i) {
                            conv(ConvCall(M.fuse[i][j][0], xs[j].p, N, xs[j].H, xs[j].W, o.p, o.ld, o.H, o.W).add(res, o.ld).act(term_act).f16(h16).upsample(j - i).filled());
                        } else {   // i - j stride-2 convs; the last one writes the term
                            const std::vector<Layer> &ls = M.fuse[i][j];
                            const Map tmp = down_chain(ls, ls.size() - 1, xs[j]);
                            conv(ConvCall(ls.back(), tmp.p ? tmp : xs[j], o).s(2).pad(1).add(res, o.ld).act(term_act).f16(h16).filled());
                            release(tmp);
                        }
                        if (!first) release(running);
                        running = o;
                        ++nterm;
                    }
                    if (fused) {
                        Map o = act(N, xi.H, xi.W, xi.C);
                        fp.base = running.p ? running.p : xi.p;
                        fp.out = o.p;
                        for (int q = 0; q < fp.nsrc; ++q) fp.src[q].x = xs[i + 1 + q].p;
                        hr_fuse_up(fp, M.fuse[i][i + 1][0].label + "+up");
                        release(running);
                        running = o;
                    }
                    outs[i] = running;
                }
                for (int b = 0; b < nbr; ++b) { release(xs[b]); xs[b] = outs[b]; }
            }
            npre = nbr;
            for (int i = 0; i < nbr; ++i) { pre[i] = xs[i]; xs[i] = Map(); }
        }
        Features f;
        f.n = 4;
        for (int i = 0; i < 4; ++i) f.lv[i] = pre[i];
        capture_feat0(f.lv[0]);
        // pose_net = Conv2d(C0, 21, 3, stride 2, padding 1) on the highest-resolution branch (handmvnet.py:51-57, 180)
        f.hm = f32map(N, conv_out(f.lv[0].H, 3, 2, 1), conv_out(f.lv[0].W, 3, 2, 1), NJ, 32);
        conv(ConvCall(h->pose0, f.lv[0], f.hm).s(2).pad(1));
        return f;
    }

    // ResNet-18 / 34 / 50-paper (resnet.py:216-254) and their pose_net (handmvnet.py:70-86)
    Features resnet_backbone(int N, const float *x) {
        const int H = h->cfg.height, W = h->cfg.width;
        // ---- stem: conv1 7x7 s2 + BN + ReLU, maxpool 3x3 s2 (resnet.py:218-221)
        // as a 4x4 stride-1 conv over the 2x2 space-to-depth frames: 12 fp32 / 16 fp16 (12 + 4 zeros) / [hi16 | lo16] per s2d pixel
        const int Hs = (H + 1) / 2, Ws = (W + 1) / 2, smode = split ? 2 : (h16 ? 1 : 0);
        Map in4 = act(N, Hs, Ws, 12, h16 ? 16 : 12);
        if (src && src->frames) LAUNCH(launch_frames_to_input(src->frames, src->boxes, N, src->fh, src->fw, H, W, src->mean, src->std, smode, in4.p, s, /*s2d=*/true, src->index, src->n_src, src->rects));
        else LAUNCH(launch_nchw_to_s2d(x, in4.p, N, H, W, smode, s, h->sat));
        const int H1 = conv_out(H, 7, 2, 3), W1 = conv_out(W, 7, 2, 3);   // == Hs, Ws
        const int hp = conv_out(H1, 3, 2, 1), wp = conv_out(W1, 3, 2, 1);
        // fp16, many frames: conv1 + BN + ReLU + maxpool as ONE launch (conv_hs.hip's pooled epilogue: the 64-channel conv map, 8x the
        // pooled map's bytes, never reaches HBM).  Bit-identical to the two launches, so the choice may depend on the launch size
        auto stem = [&](float *out) { return ConvCall(h->stem, in4.p, N, Hs, Ws, out, 64, H1, W1).pad(2).act(ACT_RELU).f16(h16); };
        const bool stem_pool = h16 && !split && h->chain_fuse && conv_hs_supported(params(stem(nullptr).pooled(hp, wp)), route);
        Map cur;
        if (stem_pool) {
            cur = act(N, hp, wp, 64);
            conv(stem(cur.p).pooled(hp, wp));
            release(in4);
        } else {
            Map c1 = act(N, H1, W1, 64);
            conv(stem(c1.p));
            release(in4);
            cur = act(N, hp, wp, 64);
            if (split) LAUNCH(launch_maxpool3s2_split(c1.p, cur.p, N, H1, W1, 64, hp, wp, s));
            else if (h16) LAUNCH(launch_maxpool3s2_f16(c1.p, cur.p, N, H1, W1, 64, hp, wp, s));
            else LAUNCH(launch_maxpool3s2(c1.p, cur.p, N, H1, W1, 64, hp, wp, s));
            release(c1);
        }

        // ---- residual layers (resnet.py:223-239)
        Map level[3], t1_chained;
        for (int li = 0; li < 3; ++li) {
            for (size_t bi = 0; bi < h->blocks[li].size(); ++bi) {
                const Block &b = h->blocks[li][bi];
                // the block behind this one (of this layer or the first of the next): its conv1 may ride on this block's conv3 launch
                const Block *nb = bi + 1 < h->blocks[li].size() ? &h->blocks[li][bi + 1] : (li + 1 < 3 && !h->blocks[li + 1].empty() ? &h->blocks[li + 1][0] : nullptr);
                Map y = h->paper ? bottleneck(b, cur, nb, t1_chained) : basic_block(b.c1, b.c2, b.has_ds ? &b.ds : nullptr, b.stride, cur, /*fill=*/false);
                bool keep = false;
                for (int q = 0; q < 3; ++q) keep |= (level[q].p == cur.p);
                if (!keep) release(cur);
                cur = y;
            }
            // handmvnet.py:165-177: feats = [layer3, layer2, layer1][:n_levels]; keep only what is sampled
            const bool needed = (li == 2) || (2 - li) < h->cfg.n_levels;
            if (needed) level[li] = cur;
        }
        Features f;
        for (int li = 2; li >= 0; --li)   // feats = [layer3, layer2, layer1]; only the kept levels are non-null
            if (level[li].p) f.lv[f.n++] = level[li];
        const Map &feat0 = f.lv[0];
        capture_feat0(feat0);

        // ---- pose_net (handmvnet.py:70-86, 180) -> channels-last heat map with row stride 32
        if (h->paper) {
            Map ph = act(N, feat0.H, feat0.W, 512);
            conv(ConvCall(h->pose0, feat0, ph).act(ACT_RELU).f16(h16));
            f.hm = f32map(N, feat0.H, feat0.W, NJ, 32);   // heat-map logits are ALWAYS fp32 (x1000 temperature)
            conv(ConvCall(h->pose1, ph, f.hm));
            release(ph);
        } else {
            const int fh = feat0.H, fw = feat0.W;
            Map p0 = act(N, 2 * fh, 2 * fw, 128);
            if (h->deconv_all.w)
                conv(ConvCall(h->deconv_all, feat0.p, N, fh, fw, p0.p, 128, fh, fw).pad(1).act(ACT_RELU).f16(h16).all_phases(4, h->deconv_stride));
            else
                for (int a = 0; a < 2; ++a)
                    for (int b = 0; b < 2; ++b)
                        conv(ConvCall(h->deconv[a * 2 + b], feat0.p, N, fh, fw, p0.p, 128, fh, fw).pad(1 - a, 1 - b).act(ACT_RELU).f16(h16).phase(a, b));
            Map p1 = act(N, p0.H, p0.W, 64);
            conv(ConvCall(h->pose1, p0, p1).pad(1).act(ACT_RELU).f16(h16));
            release(p0);
            f.hm = f32map(N, p0.H, p0.W, NJ, 32);
            conv(ConvCall(h->pose2, p1, f.hm).pad(1));
            release(p1);
        }
        return f;
    }

    // soft-argmax, SampleNet and the token rows (handmvnet.py:182-225): releases the backbone's maps, returns the tokens [N * 21][ldt].
    // Xpairs: those rows once more as [hi ldt | lo ldt] halfs where the first fusion block's projection reads pairs, else left as it is (null)
    float *tokens_stage(const Features &f, const float *bbox, const float *intr, float *crop_img, float *heatmap, float *&Xpairs) {
        const hmv_config &c = h->cfg;
        const int N = f.hm.N, V = c.num_views, d = h->d, ldt = h->ldt;
        // ---- soft-argmax (handmvnet.py:182, 252)
        float *coords = alloc((size_t)N * NJ * 2);
        LAUNCH(launch_soft_argmax(f.hm.p, f.hm.ld, N, f.hm.H, f.hm.W, coords, crop_img, (float)c.image_size, (float)c.heatmap_size, heatmap, s));
        release(f.hm);
        if (h->capture && !dry && !vs && !sweep && h->cap_coords)
            LAUNCH(hipMemcpyAsync(h->cap_coords, coords, (size_t)N * NJ * 2 * sizeof(float), hipMemcpyDeviceToDevice, s));

        // ---- sample nets as gather -> conv1x1+BN+ReLU -> bilinear blend (nets.py:46-63; handmvnet.py:185-187)
        float *tokens = tokens_dst ? tokens_dst : alloc((size_t)N * NJ * ldt);
        int col0 = 0;
        for (int i = 0; i < c.n_levels; ++i) {
            const Map &lv = f.lv[i];
            const int Ci = lv.ld, co = lv.C / 2;   // gather the (padded) channel rows; the conv's pad weights are zero
            float *g = alloc(ACT((size_t)N * NJ * 4 * Ci));
            // a split row is Ci (hi, lo) pairs = Ci 4-byte elements, like fp32
            LAUNCH(launch_sample_gather(lv.p, N, lv.H, lv.W, Ci, coords, g, s, (h16 && !split) ? 2 : 4));
            float *s4 = alloc((size_t)N * NJ * 4 * co);
            gemm(h->sample[i], g, N * NJ * 4, s4, co, nullptr, 0, ACT_RELU);
            release(g);
            LAUNCH(launch_sample_blend(s4, co, co, N, lv.H, lv.W, coords, tokens, ldt, col0, s));
            release(s4);
            col0 += co;
        }
        for (int i = 0; i < f.n; ++i) release(f.lv[i]);
        // pos2d / FoV / zero pad / PE (handmvnet.py:189-225; fusion.py:27-28).  In the fp16-kernel modes the q/k/v projections of
        // CrossAttentionFusion read their token rows as (hi, lo) fp16 pairs: the kernel that produces a block's input rows -- this one for
        // block 0, ff_block_kernel for the others -- writes that copy itself (rows_f32_to_half's arithmetic, one launch less per block)
        // A sweep stops before the part that depends on the camera subset: no PE, no pair copy (tokens_expand_subsets_kernel adds both per subset)
        if (!sweep && !h->lq && c.fusion_layers > 0 && h->attn[0].qkv.plane) Xpairs = alloc((size_t)N * NJ * ldt);
        const float *pe = (h->lq || !(c.pos_enc & HMV_POS_SIN)) ? nullptr : h->pe;   // the learnable-query blocks add their own PE
        if (sweep) LAUNCH(launch_tokens_finalize(tokens, ldt, d, h->fdim, N, V, coords, bbox, intr, c.pos_enc, nullptr, nullptr, s, nullptr, nullptr));
        else if (vs) LAUNCH(launch_tokens_finalize_views(tokens, ldt, d, h->fdim, N, vs->fpos, coords, bbox, intr, c.pos_enc, pe, s, Xpairs, h->sat));
        else LAUNCH(launch_tokens_finalize(tokens, ldt, d, h->fdim, N, V, coords, bbox, intr, c.pos_enc, pe,
                                           (h->capture && h->cap_tokens) ? h->cap_tokens : nullptr, s, Xpairs, h->sat));
        release(coords);
        return tokens;
    }

    // CrossAttentionFusionLearnableQuery (fusion.py:33-49; MultiHeadAttentionLearnableQuery layers.py:273-301): token rows X [B * Tcur][ldt]
    // in (released), the fused rows out; Tcur follows
    // A ragged forward (vs): up to and including the probe block a sample owns T_b = 21 v_b rows, the segment seg[b] .. seg[b + 1] of the
    // vs->N * 21 packed rows; Tcur is then the longest sample's count.  Behind the probe block every sample has 21 rows, as ever.
    float *fusion_learnable_query(int B, float *X, int &Tcur) {
        const int d = h->d, ldt = h->ldt;
        for (int l = 0; l < 5; ++l) {
            const AttnLayer &a = h->attn[l];
            const bool cross = l == 2, ragged = vs && l <= 2;
            const int rows = ragged ? vs->N * NJ : B * Tcur, Tq = cross ? NJ : Tcur, qrows = (ragged && !cross) ? rows : B * Tq;
            float *xp = alloc((size_t)rows * ldt);                       // x = self.pos_embed(x)
            if (ragged) LAUNCH(launch_add_pe_views(X, ldt, rows, vs->fpos, d, h->pe, xp, ldt, s));
            else LAUNCH(launch_add_pe(X, ldt, rows, Tcur, d, h->pe, xp, ldt, s));
            release(X);
            float *att = alloc((size_t)qrows * INNER_LQ);
            const bool tx3 = a.out_x3.plane != 0 && ff_fusable(a, qrows, true);   // attention rows as (hi, lo) pairs
            if (cross) {
                float *kv = alloc((size_t)rows * 2 * INNER_LQ);
                project(a.kv, xp, rows, kv, 2 * INNER_LQ);
                if (ragged) LAUNCH(launch_attention_d256_views(a.qprobe, INNER_LQ, 0, kv, kv + INNER_LQ, 2 * INNER_LQ, B, vs->seg, Tcur, att, s, tx3 ? 1 : 0, h->sat));
                else LAUNCH(launch_attention_d256(a.qprobe, INNER_LQ, 0, kv, kv + INNER_LQ, 2 * INNER_LQ, B, Tcur, Tq, att, s, tx3 ? 1 : 0, h->sat));
                attention_map(l, 2, a.qprobe, INNER_LQ, kv, 2 * INNER_LQ, B,
                              ragged ? AttnProbsRows{vs->seg, 0, 0, NJ, 0, 0, 0, 0, NJ, Tcur} : AttnProbsRows{nullptr, 0, 0, 0, Tcur, Tq, Tcur, 0, NJ, Tcur},
                              0, Tcur / NJ);
                release(kv);
            } else {
                float *qkv = alloc((size_t)rows * 3 * INNER_LQ);
                project(a.qkv, xp, rows, qkv, 3 * INNER_LQ);
                if (ragged) LAUNCH(launch_attention_d256_views(qkv, 3 * INNER_LQ, 1, qkv + INNER_LQ, qkv + 2 * INNER_LQ, 3 * INNER_LQ, B, vs->seg, Tcur, att, s, tx3 ? 1 : 0, h->sat));
                else LAUNCH(launch_attention_d256(qkv, 3 * INNER_LQ, Tcur, qkv + INNER_LQ, qkv + 2 * INNER_LQ, 3 * INNER_LQ, B, Tcur, Tq, att, s, tx3 ? 1 : 0, h->sat));
                attention_map(l, 2, qkv, 3 * INNER_LQ, qkv + INNER_LQ, 3 * INNER_LQ, B,
                              ragged ? AttnProbsRows{vs->seg, 1, 0, 0, 0, 0, 0, 0, Tcur, Tcur} : AttnProbsRows{nullptr, 0, 0, 0, Tcur, Tq, Tcur, Tcur, Tcur, Tcur},
                              0, l < 2 ? Tcur / NJ : 0);
                release(qkv);
            }
            if (ff_fusable(a, qrows, tx3)) {
                // out = to_out(att) (+ x, not in the probe block); out = ff(out) + out: no LayerNorm around the attention, the
                // FeedForward keeps its own; pad columns come out as zeros
                float *Xf = alloc((size_t)qrows * ldt);
                ff_block(a, att, qrows, cross ? nullptr : xp, 0, 0, Xf, nullptr, tx3);
                release(att);
                release(xp);
                X = Xf;
                Tcur = Tq;
                continue;
            }
            float *o = alloc((size_t)qrows * ldt);
            if (cross) gemm(a.out, att, qrows, o, ldt, nullptr, 0, ACT_NONE);   // out = to_out(att); no residual from the tokens
            else gemm(a.out, att, qrows, o, ldt, xp, ldt, ACT_NONE);            // out = to_out(att) + x
            release(att);
            release(xp);
            float *f0 = alloc((size_t)qrows * ldt);
            LAUNCH(launch_layernorm(o, ldt, qrows, d, a.fg, a.fb, f0, ldt, nullptr, nullptr, nullptr, s));
            float *f1 = alloc((size_t)qrows * DHEAD_LQ);
            gemm(a.ff1, f0, qrows, f1, DHEAD_LQ, nullptr, 0, ACT_GELU);
            release(f0);
            float *Xn = alloc((size_t)qrows * ldt);
            gemm(a.ff2, f1, qrows, Xn, ldt, o, ldt, ACT_NONE);          // out = ff(out) + out
            release(f1);
            release(o);
            // The decoder's GEMM reads all ldt columns of the last block's output (its weights are zero there, but 0 * NaN is NaN)
            // and no epilogue writes them: a GEMM epilogue stops at round4(d), the split-K reduction at d.  Inner blocks go
            // through add_pe, which writes the pad itself.
            if (l == 4 && ldt > d) LAUNCH(hipMemset2DAsync(Xn + d, (size_t)ldt * sizeof(float), 0, (size_t)(ldt - d) * sizeof(float), (size_t)qrows, s));
            X = Xn;
            Tcur = Tq;
        }
        return X;
    }

    // CrossAttentionFusion (fusion.py:7-30; layers.py:202-237): as above; Xpairs: the (hi, lo) pair copy of X where tokens_stage wrote one
    float *fusion_cross_attn(int B, float *X, float *Xpairs, int &Tcur) {
        const hmv_config &c = h->cfg;
        const int d = h->d, ldt = h->ldt;
        const int half = (c.fusion_layers - 1) / 2;
        for (int l = 0; l < c.fusion_layers; ++l) {
            const AttnLayer &a = h->attn[l];
            const bool cross = (l == half), ragged = vs && l <= half;   // (as in fusion_learnable_query)
            const int Tq = cross ? NJ : Tcur, koff = cross ? NJ : 0, Tk = cross ? Tcur - NJ : Tcur;
            const int rows = ragged ? vs->N * NJ : B * Tcur, qrows = (ragged && !cross) ? rows : B * Tq;
#ifdef HMV_NO_ATT_X3   // A/B builds only (python -m handmvnet_amd.build --variant noax HMV_NO_ATT_X3): the exact-fp32 attention in every mode
            const int att_x3 = 0;
#else
            // fp16-kernel modes: the projection writes q, k, v as (hi, lo) pairs and the attention multiplies on the fp16 matrix cores (by the
            // arithmetic mode alone: a sample's result never depends on the batch)
            const int att_x3 = (h16 && a.qkv.plane) ? 1 : 0;
#endif
            float *qkv = alloc((size_t)rows * 3 * INNER);
            project(a.qkv, X, rows, qkv, 3 * INNER, Xpairs, att_x3 != 0);
            Xpairs = nullptr;
            float *att = alloc((size_t)qrows * INNER);
            // fp16-kernel modes, fused tail: the attention rows leave the kernel as (hi, lo) pairs and to_out is a split-pair GEMM
            const bool tx3 = a.out_x3.plane != 0 && ff_fusable(a, qrows, true);
            // (ragged: a sample with one view has no keys in the cross block; the kernel writes its rows as zeros)
            if (ragged) LAUNCH(launch_attention_views(qkv, B, vs->seg, Tcur, cross ? 1 : 0, att, s, tx3 ? 1 : 0, att_x3, h->sat));
            else if (Tk > 0) LAUNCH(launch_attention(qkv, B, Tcur, Tq, koff, Tk, att, s, tx3 ? 1 : 0, att_x3, h->sat));
            else LAUNCH(hipMemsetAsync(att, 0, (size_t)qrows * INNER * sizeof(float), s));   // (zero rows are zero pairs)
            {   // (pair rows [hi 3072 | lo 3072]: strides and offsets in halfs)
                const int ld = att_x3 ? 6 * INNER : 3 * INNER;
                const void *kp = att_x3 ? static_cast<const void *>(reinterpret_cast<const _Float16 *>(qkv) + INNER) : static_cast<const void *>(qkv + INNER);
                attention_map(l, att_x3, qkv, ld, kp, ld, B,
                              ragged ? AttnProbsRows{vs->seg, 1, koff, cross ? NJ : 0, 0, 0, 0, 0, Tq, Tk} : AttnProbsRows{nullptr, 0, koff, 0, Tcur, Tq, Tk, Tcur, Tq, Tk},
                              cross ? 1 : 0, l <= half ? Tcur / NJ : 0);
            }
            release(qkv);
            // ragged cross block: the residual `_q` = each sample's first 21 rows, gathered into contiguous rows, so that everything
            // behind the attention addresses its residual row by row (rg_out = 0) as in the self blocks
            int rgo = cross ? Tq : 0, rgi = cross ? Tcur : 0;
            if (ragged && cross) {
                float *Xq = alloc((size_t)qrows * ldt);
                LAUNCH(launch_gather_query_rows(X, ldt, vs->seg, B, Xq, s));
                release(X);
                X = Xq;
                rgo = rgi = 0;
            }
            if (ff_fusable(a, qrows, tx3)) {   // norm1(to_out + _q) -> FeedForward -> norm2 in one launch behind the GEMM
                float *Xf = alloc((size_t)qrows * ldt);
                if (l + 1 < c.fusion_layers && h->attn[l + 1].qkv.plane) Xpairs = alloc((size_t)qrows * ldt);   // the next block's projection input
                ff_block(a, att, qrows, X, rgo, rgi, Xf, Xpairs, tx3);
                release(att);
                release(X);
                X = Xf;
                Tcur = Tq;
                continue;
            }
            float *n1 = alloc((size_t)qrows * ldt), *f0 = alloc((size_t)qrows * ldt);
            gemm_ln(a.out, att, qrows, X, ldt, rgo, rgi, a.n1g, a.n1b, n1, ldt, a.fg, a.fb, f0);  // norm1(to_out + _q), ff LN
            release(att);
            float *f1 = alloc((size_t)qrows * DHEAD);
            gemm(a.ff1, f0, qrows, f1, DHEAD, nullptr, 0, ACT_GELU);
            release(f0);
            float *f2 = alloc((size_t)qrows * ldt);
            gemm(a.ff2, f1, qrows, f2, ldt, n1, ldt, ACT_NONE);
            release(f1);
            float *Xn = alloc((size_t)qrows * ldt);
            LAUNCH(launch_layernorm(f2, ldt, qrows, d, a.n2g, a.n2b, Xn, ldt, nullptr, nullptr, nullptr, s));
            release(f2);
            release(n1);
            release(X);
            X = Xn;
            Tcur = Tq;
        }
        return X;
    }

    // decoder (nets.py:133-139 / 150-154): the fused rows X [B * 21][ldt] (released) -> joints_cam [B * 21][3]
    void decoder(int B, float *X, float *joints_cam) {
        const hmv_config &c = h->cfg;
        const int d = h->d, ldt = h->ldt, jr = B * NJ;
        if (c.decoder == HMV_DECODER_GCN && h->cheb_fuse && h->gcn[0].Kpad == ldt &&
            cheb_fusable(ldt, ldt, h->gcn[0].Kpad, 256, h->gcn[1].Kpad, 64, h->gcn[2].Kpad, 3)) {
            // the three ChebConv layers in two launches (fusion_kernels.hip): layer 1 per (sample, 16 channels), layers 2 + 3 per sample
            float *scr = alloc((size_t)jr * 256);
            launch("cheb_fused", [&] {
                ChebFusedParams p{};
                p.x = X; p.ldx = ldt; p.B = B; p.K = ldt;
                p.w1 = h->gcn[0].w; p.ldw1 = h->gcn[0].Kpad; p.c1 = 256; p.bias1 = h->gcn_bias[0];
                p.w2 = h->gcn[1].w; p.ldw2 = h->gcn[1].Kpad; p.c2 = 64; p.bias2 = h->gcn_bias[1];
                p.w3 = h->gcn[2].w; p.ldw3 = h->gcn[2].Kpad; p.c3 = 3; p.bias3 = h->gcn_bias[2];
                p.tk = h->cheb_t; p.scratch = scr; p.out = joints_cam; p.ldo = 3;
                return launch_cheb_fused(p, s);
            }, 2);
            release(X);
            release(scr);
        } else if (c.decoder == HMV_DECODER_GCN) {
            const int dims[4] = {d, 256, 64, 3};
            float *xin = X;
            for (int i = 0; i < 3; ++i) {
                const int co = dims[i + 1];
                float *y = alloc((size_t)jr * 3 * co);
                gemm(h->gcn[i], xin, jr, y, 3 * co, nullptr, 0, ACT_NONE);
                release(xin);
                float *out = i == 2 ? joints_cam : alloc((size_t)jr * co);
                LAUNCH(launch_cheb_mix(y, 3 * co, B, co, h->cheb_t, h->gcn_bias[i], i < 2, out, i == 2 ? 3 : co, s));
                release(y);
                xin = i == 2 ? nullptr : out;
            }
        } else {
            float *g1 = alloc((size_t)jr * 64);
            gemm(h->fc1, X, jr, g1, 64, nullptr, 0, ACT_LEAKY);
            release(X);
            gemm(h->fc2, g1, jr, joints_cam, 3, nullptr, 0, ACT_NONE);
            release(g1);
        }
    }
};
#undef LAUNCH

// the second stream of the HRNet branch overlap, made by the first real forward that needs it
int ensure_aux_stream(hmv_engine *h) {
    if (h->hrnet && h->hr_overlap && h->cfg.dtype != HMV_F32 && !h->aux) {   // (the first forward of a handle is never a captured one)
        if (hipStreamCreateWithFlags(&h->aux, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess)
            return h->fail(HMV_ERR_HIP, "second stream for the HRNet branches");
    }
    return HMV_OK;
}

// HandMvNet.forward (handmvnet.py:158-266), stage by stage; a planning run (dry) issues the same alloc / release sequence and launches nothing
// vs (ragged view sets, hmv_forward_views): the backbone and the token stage run on vs->N frames, the fusion over each sample's own rows
int run_forward(hmv_engine *h, const ForwardCall &fc, bool dry, Arena &A, const ViewSet *vs = nullptr) {
    Runner R{h, fc.stream, dry, HMV_OK, A, vs, false, &fc.src};
    const hmv_config &c = h->cfg;
    if (!dry)
        if (const int rc = ensure_aux_stream(h)) return rc;
    const int B = fc.batch, N = vs ? vs->N : B * c.num_views;
    const Features f = h->hrnet ? R.hrnet_backbone(N, fc.x) : R.resnet_backbone(N, fc.x);
    float *Xpairs = nullptr;
    float *X = R.tokens_stage(f, fc.bbox, fc.intrinsic, fc.joints_crop_img, fc.heatmap, Xpairs);
    int Tcur = vs ? vs->Tmax : c.num_views * NJ;
    X = h->lq ? R.fusion_learnable_query(B, X, Tcur) : R.fusion_cross_attn(B, X, Xpairs, Tcur);
    if (h->capture && !dry && !vs && h->cap_fused) R.launch("copy_rows", [&] { return launch_copy_rows(X, h->ldt, h->cap_fused, h->d, B * Tcur, h->d, fc.stream); });
    R.decoder(B, X, fc.joints_cam);
    return R.rc;
}

// One fusion pass of a camera-subset sweep (hmv_forward_subsets).  Virtual sample q is sample q % B under subset q / B; the pass takes the
// virtual samples q0 .. q0 + nv, n packed frames in all, at most vmax cameras in one.  Its tables start `tab` entries into the call's
// table: [seg: nv + 1 | fpos: n | src: n], seg and fpos as a ViewSet's, src[m] = the frame b * V + camera that packed frame m repeats.
struct SubsetChunk { int q0, nv, n, vmax; size_t tab; };

// The sweep: backbone and token stage ONCE on all B * V frames -- the rows [B * V * 21][ldt] stay, finalised without PE -- then per chunk the
// packed rows of its virtual samples (tokens_expand_subsets_kernel) and the unchanged ragged fusion and decoder over them, which write
// joints_cam[q0 .. q0 + nv).  tab: the call's device table (null in a planning run).  Per-sample arithmetic never depends on a size, so a
// subset's bits do not depend on the chunks.  While profiling, one bracketing record around the per-frame stage ("subsets_frames") and one
// around every pass ("subsets_tail") besides the launches' own.
int run_forward_subsets(hmv_engine *h, const ForwardCall &fc, const std::vector<SubsetChunk> &chunks, const int32_t *tab, bool dry, Arena &A) {
    Runner R{h, fc.stream, dry, HMV_OK, A, nullptr, true, &fc.src};
    const hmv_config &c = h->cfg;
    const hipStream_t s = fc.stream;
    float *const joints_cam = fc.joints_cam;
    if (!dry)
        if (const int rc = ensure_aux_stream(h)) return rc;
    auto bracket_begin = [&](const char *label) {   // (an index: nested records may move the list)
        if (!h->profiling || dry) return (size_t)-1;
        R.prof_begin(label);
        return h->prof_used - 1;
    };
    auto bracket_end = [&](size_t i, const char *name) {
        if (i == (size_t)-1) return;
        h->prof[i].flops = h->prof[i].bytes = 0;
        R.prof_end(&h->prof[i], name);
    };
    const int N = fc.batch * c.num_views, ldt = h->ldt;
    size_t br = bracket_begin("frames");
    const Features f = h->hrnet ? R.hrnet_backbone(N, fc.x) : R.resnet_backbone(N, fc.x);
    float *no_pairs = nullptr;
    float *rows = R.tokens_stage(f, fc.bbox, fc.intrinsic, fc.joints_crop_img, fc.heatmap, no_pairs);
    bracket_end(br, "subsets_frames");
    const bool want_pairs = !h->lq && c.fusion_layers > 0 && h->attn[0].qkv.plane;   // (as tokens_stage decides for a forward)
    const float *pe = (h->lq || !(c.pos_enc & HMV_POS_SIN)) ? nullptr : h->pe;
    for (const SubsetChunk &ck : chunks) {
        br = bracket_begin("tail");
        const int32_t *t = tab ? tab + ck.tab : nullptr;
        const ViewSet vs{ck.n, t, t ? t + ck.nv + 1 : nullptr, NJ * ck.vmax};
        const int32_t *src = t ? t + ck.nv + 1 + ck.n : nullptr;
        float *X = R.alloc((size_t)ck.n * NJ * ldt);
        float *Xpairs = want_pairs ? R.alloc((size_t)ck.n * NJ * ldt) : nullptr;
        R.launch("tokens_expand_subsets", [&] { return launch_tokens_expand_subsets(rows, ldt, h->d, ck.n, src, vs.fpos, pe, X, Xpairs, s, h->sat); });
        R.vs = &vs;
        int Tcur = vs.Tmax;
        X = h->lq ? R.fusion_learnable_query(ck.nv, X, Tcur) : R.fusion_cross_attn(ck.nv, X, Xpairs, Tcur);
        R.decoder(ck.nv, X, joints_cam ? joints_cam + (size_t)ck.q0 * NJ * 3 : nullptr);
        R.vs = nullptr;
        bracket_end(br, "subsets_tail");
    }
    R.release(rows);
    return R.rc;
}

// An occlusion sweep (hmv_forward_frames_occlusions), planned on the host.  Occluded frame q = o * B + b is frame b * V + occ_view[o] under
// the rectangle rects[q]; the frame stage takes them in `passes` (frames q0 .. q0 + n), the tail runs in `chunks` of virtual samples
// (1 + n_occ) * B in all: sample b clean, then sample b under variant o).  The call's device table is [index: n_occ * B | the chunks' tables as
// a subset sweep's], index[q] = the slot b * V + occ_view[o].
struct OccPass { int q0, n; };
struct OccPlan {
    int n_occ = 0;
    std::vector<OccPass> passes;
    std::vector<SubsetChunk> chunks;
    const int32_t *rects = nullptr;                // device [n_occ * B][4]
    float *crop_occ = nullptr, *hm_occ = nullptr;  // the occluded camera's own 2D output, [n_occ * B][21][2] and [n_occ * B][21][H/8][W/8], or null
};

// The sweep: the per-frame stage in sweep form (rows without PE and pair copy) on the B * V clean frames, then on the occluded frames pass by
// pass, all into ONE retained block of token rows [(B * V + n_occ * B) * 21][ldt]; then, as in run_forward_subsets, per chunk the packed rows
// of its virtual samples and the unchanged ragged fusion and decoder.  Every virtual sample has all V views, so its bits are those of a
// uniform forward on the frames it stands for.  While profiling, bracketing records "occlusions_frames" (the clean stage, every occluded
// pass) and "occlusions_tail" (every tail pass).
int run_forward_occlusions(hmv_engine *h, const ForwardCall &fc, const OccPlan &op, const int32_t *tab, bool dry, Arena &A) {
    Runner R{h, fc.stream, dry, HMV_OK, A, nullptr, true, &fc.src};
    const hmv_config &c = h->cfg;
    const hipStream_t s = fc.stream;
    if (!dry)
        if (const int rc = ensure_aux_stream(h)) return rc;
    auto bracket_begin = [&](const char *label) {   // (an index: nested records may move the list)
        if (!h->profiling || dry) return (size_t)-1;
        R.prof_begin(label);
        return h->prof_used - 1;
    };
    auto bracket_end = [&](size_t i, const char *name) {
        if (i == (size_t)-1) return;
        h->prof[i].flops = h->prof[i].bytes = 0;
        R.prof_end(&h->prof[i], name);
    };
    const int B = fc.batch, V = c.num_views, N = B * V, M = op.n_occ * B, ldt = h->ldt;
    size_t hm_frame = 0;   // floats of one frame's heat-maps
    float *rows = R.alloc((size_t)(N + M) * NJ * ldt);
    float *no_pairs = nullptr;
    size_t br = bracket_begin("frames");
    {
        R.tokens_dst = rows;
        const Features f = h->hrnet ? R.hrnet_backbone(N, nullptr) : R.resnet_backbone(N, nullptr);
        hm_frame = (size_t)NJ * f.hm.H * f.hm.W;
        R.tokens_stage(f, fc.bbox, fc.intrinsic, fc.joints_crop_img, fc.heatmap, no_pairs);
    }
    bracket_end(br, "occlusions_frames");
    const bool crop_pe = (c.pos_enc & HMV_POS_CROP) != 0;
    for (const OccPass &ps : op.passes) {
        br = bracket_begin("occluded");
        FrameSrc src = fc.src;
        src.index = tab ? tab + ps.q0 : nullptr;
        src.n_src = N;
        src.rects = op.rects ? op.rects + (size_t)ps.q0 * 4 : nullptr;
        R.src = &src;
        R.tokens_dst = rows + (size_t)(N + ps.q0) * NJ * ldt;
        // the slot's bbox and intrinsic rows (the crop-FoV columns of the token rows)
        float *bb = crop_pe ? R.alloc((size_t)ps.n * 4) : nullptr, *in = crop_pe ? R.alloc((size_t)ps.n * 4) : nullptr;
        if (crop_pe) R.launch("gather_rows4", [&] { return launch_gather_rows4(fc.bbox, fc.intrinsic, src.index, ps.n, N, bb, in, s); });
        float *crop = op.crop_occ ? op.crop_occ + (size_t)ps.q0 * NJ * 2 : R.alloc((size_t)ps.n * NJ * 2);
        const Features f = h->hrnet ? R.hrnet_backbone(ps.n, nullptr) : R.resnet_backbone(ps.n, nullptr);
        R.tokens_stage(f, bb, in, crop, op.hm_occ ? op.hm_occ + (size_t)ps.q0 * hm_frame : nullptr, no_pairs);
        if (!op.crop_occ) R.release(crop);
        R.release(in);
        R.release(bb);
        R.src = &fc.src;
        bracket_end(br, "occlusions_frames");
    }
    R.tokens_dst = nullptr;
    const bool want_pairs = !h->lq && c.fusion_layers > 0 && h->attn[0].qkv.plane;   // (as tokens_stage decides for a forward)
    const float *pe = (h->lq || !(c.pos_enc & HMV_POS_SIN)) ? nullptr : h->pe;
    for (const SubsetChunk &ck : op.chunks) {
        br = bracket_begin("tail");
        const int32_t *t = tab ? tab + ck.tab : nullptr;
        const ViewSet vs{ck.n, t, t ? t + ck.nv + 1 : nullptr, NJ * ck.vmax};
        const int32_t *src = t ? t + ck.nv + 1 + ck.n : nullptr;
        float *X = R.alloc((size_t)ck.n * NJ * ldt);
        float *Xpairs = want_pairs ? R.alloc((size_t)ck.n * NJ * ldt) : nullptr;
        R.launch("tokens_expand_subsets", [&] { return launch_tokens_expand_subsets(rows, ldt, h->d, ck.n, src, vs.fpos, pe, X, Xpairs, s, h->sat); });
        R.vs = &vs;
        int Tcur = vs.Tmax;
        X = h->lq ? R.fusion_learnable_query(ck.nv, X, Tcur) : R.fusion_cross_attn(ck.nv, X, Xpairs, Tcur);
        R.decoder(ck.nv, X, fc.joints_cam ? fc.joints_cam + (size_t)ck.q0 * NJ * 3 : nullptr);
        R.vs = nullptr;
        bracket_end(br, "occlusions_tail");
    }
    R.release(rows);
    return R.rc;
}

int ensure_capture(hmv_engine *h, int B) {
    if (!h->capture || h->cap_batch >= B) return HMV_OK;
    const hmv_config &c = h->cfg;
    const int N = B * c.num_views;
    // size of feats[0] by the backbones' conv arithmetic (any frame size): 3x3 s2 p1 (and 7x7 s2 p3, 1x1 s2) all give (n - 1) / 2 + 1
    auto half_up = [](int n) { return (n - 1) / 2 + 1; };
    int fh = half_up(half_up(c.height)), fw = half_up(half_up(c.width));           // stem: H/4
    if (!h->hrnet) { fh = half_up(fh); fw = half_up(fw); }                         // layer2
    if (!h->hrnet && !h->paper) { fh = half_up(fh); fw = half_up(fw); }            // layer3 of ResNet-18/34
    for (float **p : {&h->cap_feat0, &h->cap_coords, &h->cap_tokens, &h->cap_fused}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    h->cap_feat0_n = (size_t)N * c.channels[0] * fh * fw;
    h->cap_coords_n = (size_t)N * NJ * 2;
    h->cap_tokens_n = (size_t)N * NJ * h->d;
    h->cap_fused_n = (size_t)B * NJ * h->d;
    HIPCHK(h, hipMalloc(reinterpret_cast<void **>(&h->cap_feat0), h->cap_feat0_n * sizeof(float)));
    HIPCHK(h, hipMalloc(reinterpret_cast<void **>(&h->cap_coords), h->cap_coords_n * sizeof(float)));
    HIPCHK(h, hipMalloc(reinterpret_cast<void **>(&h->cap_tokens), h->cap_tokens_n * sizeof(float)));
    HIPCHK(h, hipMalloc(reinterpret_cast<void **>(&h->cap_fused), h->cap_fused_n * sizeof(float)));
    h->cap_batch = B;
    return HMV_OK;
}

// The buffers of the selected blocks' attention maps, for B full-view samples (no ragged batch of B samples needs more of any): blocks in
// front of the cross block attend over all 21 V tokens, the cross block's 21 queries over the other views' tokens (cross_attn) or over all of
// them (the learnable probe), the blocks behind it over the 21 fused tokens.  Only the blocks up to the cross block have views to share among.
int ensure_attention(hmv_engine *h, int B) {
    if (!h->att_mask || (h->att_alloc_mask == h->att_mask && h->att_batch >= B)) return HMV_OK;
    B = std::max(B, h->att_batch);
    const int V = h->cfg.num_views, cx = h->cross_block();
    h->att.resize((size_t)h->fusion_blocks());
    for (int l = 0; l < h->fusion_blocks(); ++l) {
        hmv_engine::AttMap &m = h->att[(size_t)l];
        for (float **p : {&m.probs, &m.share}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        m = hmv_engine::AttMap();
        if (!((h->att_mask >> l) & 1u)) continue;
        const size_t Tq = l == cx ? NJ : (l < cx ? (size_t)NJ * V : NJ);
        const size_t Tk = l < cx ? (size_t)NJ * V : (l == cx ? (size_t)NJ * (h->lq ? V : V - 1) : NJ);
        m.probs_cap = (size_t)B * 8 * Tq * Tk;
        m.share_cap = l <= cx ? (size_t)B * 8 * Tq * V : 0;
        HIPCHK(h, hipMalloc(reinterpret_cast<void **>(&m.probs), (m.probs_cap ? m.probs_cap : 1) * sizeof(float)));
        HIPCHK(h, hipMalloc(reinterpret_cast<void **>(&m.share), (m.share_cap ? m.share_cap : 1) * sizeof(float)));
    }
    h->att_batch = B;
    h->att_alloc_mask = h->att_mask;
    return HMV_OK;
}

// ------------------------------------------------------------------ what the forward entries share
int check_handle(hmv_handle h) {
    if (!h) return HMV_ERR_ARG;
    if (!h->finalized) return h->fail(HMV_ERR_STATE, "hmv_finalize_weights has not succeeded on this handle");
    return HMV_OK;
}

int check_crop_pe(hmv_handle h, const float *bbox, const float *intrinsic) {
    if ((h->cfg.pos_enc & HMV_POS_CROP) && (!bbox || !intrinsic))
        return h->fail(HMV_ERR_ARG, "pos_enc contains 'crop': bbox and cam_params['intrinsic'] are required");
    return HMV_OK;
}

// a call from raw frames: frames / mean / std / frame size (batch and the outputs share the first text)
int check_frames(hmv_handle h, int32_t batch, const uint8_t *frames, int32_t frame_h, int32_t frame_w, const int32_t *crop_boxes,
                 const float *mean, const float *std, const float *joints_crop_img, const float *joints_cam) {
    if (batch <= 0 || !frames || !crop_boxes || !mean || !std || !joints_crop_img || !joints_cam)
        return h->fail(HMV_ERR_ARG, "null or empty input/output");
    if (frame_h <= 0 || frame_w <= 0) return h->fail(HMV_ERR_ARG, "frame size must be positive");
    for (int c = 0; c < 3; ++c)
        if (!(std[c] > 0.f)) return h->fail(HMV_ERR_ARG, "std must be positive");
    return HMV_OK;
}

int check_views(hmv_handle h, const char *who, int32_t batch, const int32_t *view_counts, const float *bbox, const float *intrinsic) {
    if (batch <= 0) return h->fail(HMV_ERR_ARG, "%s: batch must be positive (got %d)", who, (int)batch);
    if (!view_counts) return h->fail(HMV_ERR_ARG, "%s: view_counts is null (one host entry per sample)", who);
    const int V = h->cfg.num_views;
    for (int b = 0; b < batch; ++b) {
        const int v = view_counts[b];
        if (v < 1 || v > V)
            return h->fail(HMV_ERR_ARG, "%s: view_counts[%d] = %d, every sample needs between 1 and num_views = %d present views", who, b, v, V);
    }
    return check_crop_pe(h, bbox, intrinsic);
}

FrameSrc frame_src(const uint8_t *frames, int fh, int fw, const int *boxes, const int *index, int n_src, const float *mean, const float *std) {
    FrameSrc f{frames, boxes, index, n_src, fh, fw};
    for (int c = 0; c < 3; ++c) { f.mean[c] = mean[c]; f.std[c] = std[c]; }
    return f;
}

// The next slot of the ring of pinned host tables, free to be rewritten (the upload that last read it has run) and with room for tab_n entries
int views_slot(hmv_handle h, size_t tab_n, hmv_engine::ViewsSlot *&out) {
    hmv_engine::ViewsSlot &slot = h->views_host[h->views_next++ % 4];
    if (slot.done) HIPCHK(h, hipEventSynchronize(slot.done));
    else HIPCHK(h, hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));
    if (tab_n > slot.cap) {
        if (slot.host) HIPCHK(h, hipHostFree(slot.host));
        slot.host = nullptr;
        slot.cap = 0;
        const size_t cap = std::max<size_t>(tab_n, (size_t)h->reserved_batch * (h->cfg.num_views + 1) + 1);
        HIPCHK(h, hipHostMalloc(reinterpret_cast<void **>(&slot.host), cap * sizeof(int32_t), hipHostMallocDefault));
        slot.cap = cap;
    }
    out = &slot;
    return HMV_OK;
}

// A call whose own plan needs more than the reserved workspace (checked before anything is launched): the workspace grows
int grow_workspace(hmv_handle h, size_t need) {
    if (need <= h->arena_bytes) return HMV_OK;
    HIPCHK(h, hipDeviceSynchronize());
    h->drop_graphs();   // captured launches point into the old workspace
    if (h->arena) HIPCHK(h, hipFree(h->arena));
    h->arena = nullptr;
    h->arena_bytes = 0;
    const int served = h->reserved_batch;   // the larger workspace still serves as many uniform samples
    h->reserved_batch = 0;
    HIPCHK(h, hipMalloc(reinterpret_cast<void **>(&h->arena), need));
    h->arena_bytes = need;
    h->reserved_batch = served;
    return HMV_OK;
}

// The tables of a ragged call or a sweep: tab_n entries in a slot of the pinned ring
struct ViewsUpload { hmv_engine::ViewsSlot *slot; size_t tab_n; };

// ... to the device table, on the caller's stream
int upload_views(hmv_handle h, const ViewsUpload &up, hipStream_t s) {
    if (up.tab_n > h->views_cap) {   // (hipFree waits for the launches that still read the old table)
        if (h->views_dev) HIPCHK(h, hipFree(h->views_dev));
        h->views_dev = nullptr;
        h->views_cap = 0;
        const size_t cap = std::max<size_t>(up.tab_n, (size_t)h->reserved_batch * (h->cfg.num_views + 1) + 1);
        HIPCHK(h, hipMalloc(reinterpret_cast<void **>(&h->views_dev), cap * sizeof(int32_t)));
        h->views_cap = cap;
    }
    HIPCHK(h, hipMemcpyAsync(h->views_dev, up.slot->host, up.tab_n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipEventRecord(up.slot->done, s));
    return HMV_OK;
}

// The workspace a call of `batch` samples takes: run(call, dry, arena) plans the call that carries nothing but its batch on an arena at a
// fake non-null base (offsets only).  A planning run records nothing, so profiling is off meanwhile
template <class Run> size_t plan_bytes(hmv_engine *h, int batch, Run &&run) {
    Arena dry;
    dry.reset(reinterpret_cast<char *>(uintptr_t(1) << 40));
    const bool saved = h->profiling;
    h->profiling = false;
    run(ForwardCall{batch}, /*dry=*/true, dry);
    h->profiling = saved;
    return dry.high;
}

// "Plan this call, grow the workspace if its own plan needs it, run it, check the high-water mark" in two halves; run(call, dry, arena).
// The front, for a ragged call or a sweep: the reservation for `batch` uniform samples asks for more of every buffer, but the planner is
// first-fit and these calls hold a few more small buffers, so the call's own plan is checked BEFORE anything is launched; then the tables
// go up, the call's first launch.  A uniform forward has no front: it relies on hmv_reserve, so it may run under stream capture
template <class Run> int plan_and_upload(hmv_engine *h, const ForwardCall &fc, const ViewsUpload &up, Run &&run) {
    if (const int rc = grow_workspace(h, plan_bytes(h, fc.batch, run))) return rc;
    if (const int rc = upload_views(h, up, fc.stream)) return rc;
    h->last_ragged = true;   // no stages are captured (hmv_read_stage)
    return HMV_OK;
}

// The back, for every path: the real run on the workspace, its launches counted from `first` (1 behind an upload, else 0)
template <class Run> int run_checked(hmv_engine *h, const ForwardCall &fc, int first, Run &&run) {
    h->plan.reset(h->arena);
    h->launches = first;
    const int rc = run(fc, /*dry=*/false, h->plan);
    if (rc == HMV_OK && h->plan.high > h->arena_bytes) return h->fail(HMV_ERR_STATE, "workspace plan exceeded its reservation");
    return rc;
}

// The tracking tail, on the call's stream: n_frames rows of joints move the windows of n_slots slots; index names each row's slot (null:
// row n is slot n)
int launch_track_tail(hmv_engine *h, const ForwardCall &fc, int n_frames, int n_slots, const int *index) {
    int *boxes = const_cast<int *>(fc.src.boxes);
    const TrackParams tp{n_frames, n_slots, fc.joints_crop_img, boxes, nullptr, index, h->cfg.image_size, fc.track.margin, fc.track.square,
                         boxes, const_cast<float *>(fc.bbox), fc.track.joints_img, fc.track.status};
    HIPCHK(h, launch_next_crop_boxes(tp, fc.stream));
    ++h->launches;
    return HMV_OK;
}

int forward_eager(hmv_engine *h, const ForwardCall &fc) {
    const int rc = run_checked(h, fc, 0, [h](const ForwardCall &c, bool dry, Arena &A) { return run_forward(h, c, dry, A); });
    if (rc != HMV_OK || !fc.track.on) return rc;
    const int n = fc.batch * h->cfg.num_views;
    return launch_track_tail(h, fc, n, n, nullptr);   // (under capture this launch becomes the graph's last node)
}

// The uniform forward behind hmv_forward and hmv_forward_frames(_track): the only path that may be captured and replayed
int forward_uniform(hmv_engine *h, const ForwardCall &fc) {
    if (const int rc = check_crop_pe(h, fc.bbox, fc.intrinsic)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    const int batch = fc.batch;
    if (batch > h->reserved_batch || (h->capture && h->cap_batch < batch) || (h->att_mask && (h->att_batch < batch || h->att_alloc_mask != h->att_mask)))
        if (const int rc = hmv_reserve(h, batch)) return rc;
    h->last_ragged = false;
    h->forget_attention();
    // stage capture and attention capture copy into side buffers and profiling brackets launches with events: all stay eager
    if (!h->graphs || h->capture || h->att_mask || h->profiling) return forward_eager(h, fc);

    hmv_engine::GraphKey key{};
    key[0] = (uintptr_t)batch; key[1] = (uintptr_t)fc.x; key[2] = (uintptr_t)fc.bbox; key[3] = (uintptr_t)fc.intrinsic;
    key[4] = (uintptr_t)fc.joints_crop_img; key[5] = (uintptr_t)fc.joints_cam; key[6] = (uintptr_t)fc.heatmap;
    key[7] = (uintptr_t)fc.src.frames; key[8] = (uintptr_t)fc.src.boxes;
    key[9] = ((uintptr_t)(unsigned)fc.src.fh << 32) | (uintptr_t)(unsigned)fc.src.fw;
    if (fc.src.frames) {
        uint32_t bits[6];
        memcpy(bits, fc.src.mean, 12);
        memcpy(bits + 3, fc.src.std, 12);
        key[10] = ((uintptr_t)bits[0] << 32) ^ ((uintptr_t)bits[1] << 16) ^ (uintptr_t)bits[2];
        key[11] = ((uintptr_t)bits[3] << 32) ^ ((uintptr_t)bits[4] << 16) ^ (uintptr_t)bits[5];
    }
    if (fc.track.on) {   // the tracking tail is part of the captured work: its buffers and parameters are part of the key
        key[12] = (uintptr_t)fc.track.joints_img; key[13] = (uintptr_t)fc.track.status;
        key[14] = (uintptr_t(1) << 63) | ((uintptr_t)(fc.track.square != 0) << 32) | (uintptr_t)(unsigned)fc.track.margin;
    }
    const hipStream_t s = fc.stream;
    for (auto &e : h->gcache)
        if (e.key == key) {
            e.stamp = ++h->gclock;
            ++h->greplays;
            HIPCHK(h, hipGraphLaunch(e.exec, s));
            return HMV_OK;
        }
    auto seen = std::find(h->gseen.begin(), h->gseen.end(), key);
    if (seen == h->gseen.end()) {   // first sighting: run eagerly (also configures kernels, zero page, ...)
        if (h->gseen.size() >= 16) h->gseen.erase(h->gseen.begin());
        h->gseen.push_back(key);
        return forward_eager(h, fc);
    }
    // second use of the same buffers: capture on the engine's own stream, then launch the graph on the caller's
    h->gseen.erase(seen);
    if (!h->gstream) HIPCHK(h, hipStreamCreateWithFlags(&h->gstream, hipStreamNonBlocking));
    ForwardCall captured = fc;
    captured.stream = h->gstream;
    HIPCHK(h, hipStreamBeginCapture(h->gstream, hipStreamCaptureModeThreadLocal));
    const int rc = forward_eager(h, captured);
    hipGraph_t graph = nullptr;
    const hipError_t ce = hipStreamEndCapture(h->gstream, &graph);
    hipGraphExec_t exec = nullptr;
    if (rc != HMV_OK || ce != hipSuccess || !graph || hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        if (graph) (void)hipGraphDestroy(graph);
        (void)hipGetLastError();
        h->graphs = false;   // capture is not available here: stay eager for the life of the handle
        if (rc != HMV_OK) return rc;
        return forward_eager(h, fc);
    }
    (void)hipGraphDestroy(graph);
    if (h->gcache.size() >= 8) {   // least recently replayed entry makes room
        size_t lru = 0;
        for (size_t i = 1; i < h->gcache.size(); ++i)
            if (h->gcache[i].stamp < h->gcache[lru].stamp) lru = i;
        (void)hipGraphExecDestroy(h->gcache[lru].exec);
        h->gcache.erase(h->gcache.begin() + (long)lru);
    }
    h->gcache.push_back({key, exec, ++h->gclock});
    HIPCHK(h, hipGraphLaunch(exec, s));
    return HMV_OK;
}

// The ragged forward behind hmv_forward_views and hmv_forward_frames_views(_track); the arguments have been checked.  Always eager: the
// tables differ from call to call, so a ragged call never enters the graph replay cache
int forward_ragged(hmv_engine *h, const ForwardCall &fc, const int32_t *view_counts) {
    const int batch = fc.batch;
    size_t N = 0;
    int vmax = 0;
    for (int b = 0; b < batch; ++b) {
        N += (size_t)view_counts[b];
        vmax = view_counts[b] > vmax ? view_counts[b] : vmax;
    }
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (batch > h->reserved_batch || (h->att_mask && (h->att_batch < batch || h->att_alloc_mask != h->att_mask)))
        if (const int rc = hmv_reserve(h, batch)) return rc;
    h->forget_attention();
    // the tables: [seg: B + 1 | fpos: N]
    ViewsUpload up{nullptr, (size_t)batch + 1 + N};
    if (const int rc = views_slot(h, up.tab_n, up.slot)) return rc;
    int32_t *seg = up.slot->host, *fpos = seg + batch + 1;
    seg[0] = 0;
    for (int b = 0, n = 0; b < batch; ++b) {
        seg[b + 1] = seg[b] + NJ * view_counts[b];
        for (int r = 0; r < view_counts[b]; ++r) fpos[n++] = NJ * r;
    }
    auto run = [&](const ForwardCall &c, bool dry, Arena &A) {   // (a planning run has no tables)
        const ViewSet vs{(int)N, dry ? nullptr : h->views_dev, dry ? nullptr : h->views_dev + batch + 1, NJ * vmax};
        return run_forward(h, c, dry, A, &vs);
    };
    if (const int rc = plan_and_upload(h, fc, up, run)) return rc;
    const int rc = run_checked(h, fc, 1, run);
    if (rc != HMV_OK || !fc.track.on) return rc;
    // a full-layout slot is present iff a packed frame names it: every slot starts as absent (status 1, zero joints, its window
    // untouched) and each packed row then moves the window of the slot it came from
    const int n_slots = fc.src.index ? fc.src.n_src : (int)N;
    if (fc.track.joints_img) {
        HIPCHK(h, hipMemsetAsync(fc.track.joints_img, 0, (size_t)n_slots * NJ * 2 * sizeof(float), fc.stream));
        ++h->launches;
    }
    if (fc.track.status) {
        HIPCHK(h, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(fc.track.status), 1, (size_t)n_slots, fc.stream));
        ++h->launches;
    }
    return launch_track_tail(h, fc, (int)N, n_slots, fc.src.index);
}

// hmv_forward_frames with or without a tracking tail
int forward_frames(hmv_handle h, int32_t batch, const uint8_t *frames, int32_t frame_h, int32_t frame_w, const int32_t *crop_boxes,
                   const float *mean, const float *std, const float *bbox, const float *intrinsic, float *joints_crop_img, float *joints_cam,
                   float *heatmap, const TrackTail &track, void *stream) {
    if (const int rc = check_handle(h)) return rc;
    if (const int rc = check_frames(h, batch, frames, frame_h, frame_w, crop_boxes, mean, std, joints_crop_img, joints_cam)) return rc;
    const ForwardCall fc{batch, nullptr, frame_src(frames, frame_h, frame_w, crop_boxes, nullptr, 0, mean, std), bbox, intrinsic,
                         joints_crop_img, joints_cam, heatmap, track, static_cast<hipStream_t>(stream)};
    return forward_uniform(h, fc);
}

// hmv_forward_frames_views with or without a tracking tail: the indexed frame preparation in front of the ragged forward
int forward_frames_views(hmv_handle h, int32_t batch, const int32_t *view_counts, const uint8_t *frames, int32_t frame_h, int32_t frame_w,
                         const int32_t *crop_boxes, const int32_t *frame_index, const float *mean, const float *std, const float *bbox,
                         const float *intrinsic, float *joints_crop_img, float *joints_cam, float *heatmap, const TrackTail &track,
                         void *stream) {
    if (const int rc = check_handle(h)) return rc;
    if (const int rc = check_views(h, "hmv_forward_frames_views", batch, view_counts, bbox, intrinsic)) return rc;
    if (const int rc = check_frames(h, batch, frames, frame_h, frame_w, crop_boxes, mean, std, joints_crop_img, joints_cam)) return rc;
    const ForwardCall fc{batch, nullptr, frame_src(frames, frame_h, frame_w, crop_boxes, frame_index, batch * h->cfg.num_views, mean, std),
                         bbox, intrinsic, joints_crop_img, joints_cam, heatmap, track, static_cast<hipStream_t>(stream)};
    return forward_ragged(h, fc, view_counts);
}

// S ordered camera lists over one full batch, what a sweep's fusion tails run on: list i is cams[sum count[0 .. i)) ...], count[i] distinct
// cameras in feed order (the first one is the reference view).  A subset's list is its cameras ascending (hmv_forward_subsets), an
// order's the cameras as the caller named them (hmv_forward_orders).
struct CameraLists {
    int S;
    const std::vector<int> &count, &cams;
};

// The host plan of a sweep over camera lists: the passes -- at most max(batch, reserved batch) virtual samples each, so that every
// buffer of a pass stays within the reservation -- and every pass's table [seg | fpos | src] in the slot `up` names.  Virtual sample
// q = list q / batch on sample q % batch; its frame of rank r is src = b * V + (the list's r-th camera) at position fpos = 21 r.
int plan_camera_lists(hmv_engine *h, int batch, const CameraLists &L, std::vector<SubsetChunk> &chunks, ViewsUpload &up) {
    const int V = h->cfg.num_views, total = L.S * batch, cmax = std::max<int>(batch, h->reserved_batch);
    std::vector<size_t> first(L.S + 1, 0);   // list i starts at cams[first[i]]
    for (int i = 0; i < L.S; ++i) first[i + 1] = first[i] + (size_t)L.count[i];
    for (int q0 = 0; q0 < total; q0 += cmax) {
        SubsetChunk ck{q0, std::min(cmax, total - q0), 0, 0, up.tab_n};
        for (int q = q0; q < q0 + ck.nv; ++q) {
            ck.n += L.count[q / batch];
            ck.vmax = std::max(ck.vmax, L.count[q / batch]);
        }
        up.tab_n += (size_t)ck.nv + 1 + 2 * (size_t)ck.n;
        chunks.push_back(ck);
    }
    if (const int rc = views_slot(h, up.tab_n, up.slot)) return rc;
    for (const SubsetChunk &ck : chunks) {
        int32_t *seg = up.slot->host + ck.tab, *fpos = seg + ck.nv + 1, *src = fpos + ck.n;
        seg[0] = 0;
        for (int i = 0, m = 0; i < ck.nv; ++i) {
            const int q = ck.q0 + i, list = q / batch, b = q % batch;
            seg[i + 1] = seg[i] + NJ * L.count[list];
            for (int r = 0; r < L.count[list]; ++r) { fpos[m] = NJ * r; src[m++] = b * V + L.cams[first[list] + r]; }
        }
    }
    return HMV_OK;
}

// What hmv_forward_subsets and hmv_forward_orders share behind their own argument checks: reservation, plan, upload, the eager run.
int forward_camera_lists(hmv_engine *h, const ForwardCall &fc, const CameraLists &L) {
    if (const int rc = check_crop_pe(h, fc.bbox, fc.intrinsic)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (fc.batch > h->reserved_batch)
        if (const int rc = hmv_reserve(h, fc.batch)) return rc;
    std::vector<SubsetChunk> chunks;
    ViewsUpload up{nullptr, 0};
    if (const int rc = plan_camera_lists(h, fc.batch, L, chunks, up)) return rc;
    auto run = [&](const ForwardCall &c, bool dry, Arena &A) { return run_forward_subsets(h, c, chunks, dry ? nullptr : h->views_dev, dry, A); };
    if (const int rc = plan_and_upload(h, fc, up, run)) return rc;
    h->forget_attention();   // (no attention maps either: a sweep ignores the mask)
    return run_checked(h, fc, 1, run);
}

}  // namespace

extern "C" {

size_t hmv_workspace_bytes(hmv_handle h, int32_t batch) {
    if (!h || batch <= 0) return 0;
    return plan_bytes(h, batch, [h](const ForwardCall &c, bool dry, Arena &A) { return run_forward(h, c, dry, A); });
}

int hmv_reserve(hmv_handle h, int32_t batch) {
    if (!h || batch <= 0) return h ? h->fail(HMV_ERR_ARG, "batch must be positive") : HMV_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (batch > h->reserved_batch) {
        const size_t need = hmv_workspace_bytes(h, batch);
        if (h->arena) {
            HIPCHK(h, hipDeviceSynchronize());
            h->drop_graphs();   // captured launches point into the old workspace
            HIPCHK(h, hipFree(h->arena));
            h->arena = nullptr;
        }
        HIPCHK(h, hipMalloc(reinterpret_cast<void **>(&h->arena), need));
        h->arena_bytes = need;
        h->reserved_batch = batch;
    }
    if (const int rc = ensure_capture(h, batch)) return rc;
    return ensure_attention(h, batch);
}

int hmv_set_graphs(hmv_handle h, int32_t enable) {
    if (!h) return HMV_ERR_ARG;
    (void)hipSetDevice(h->cfg.device);
    h->graphs = enable != 0;
    if (!h->graphs) { (void)hipDeviceSynchronize(); h->drop_graphs(); }
    return HMV_OK;
}

int hmv_graph_stats(hmv_handle h, int32_t *cached, int64_t *replays) {
    if (!h) return HMV_ERR_ARG;
    if (cached) *cached = (int32_t)h->gcache.size();
    if (replays) *replays = (int64_t)h->greplays;
    return HMV_OK;
}

int hmv_forward(hmv_handle h, int32_t batch, const float *x, const float *bbox, const float *intrinsic, float *joints_crop_img,
                float *joints_cam, float *heatmap, void *stream) {
    if (const int rc = check_handle(h)) return rc;
    if (batch <= 0 || !x || !joints_crop_img || !joints_cam) return h->fail(HMV_ERR_ARG, "null or empty input/output");
    const ForwardCall fc{batch, x, FrameSrc{}, bbox, intrinsic, joints_crop_img, joints_cam, heatmap, TrackTail{}, static_cast<hipStream_t>(stream)};
    return forward_uniform(h, fc);
}

/* hmv_forward for a batch whose samples have different cameras (include/handmv.h).  Everything that can be refused is refused before the
 * first launch. */
int hmv_forward_views(hmv_handle h, int32_t batch, const int32_t *view_counts, const float *x, const float *bbox, const float *intrinsic,
                      float *joints_crop_img, float *joints_cam, float *heatmap, void *stream) {
    if (const int rc = check_handle(h)) return rc;
    if (batch > 0 && view_counts && (!x || !joints_crop_img || !joints_cam)) return h->fail(HMV_ERR_ARG, "null or empty input/output");
    if (const int rc = check_views(h, "hmv_forward_views", batch, view_counts, bbox, intrinsic)) return rc;
    const ForwardCall fc{batch, x, FrameSrc{}, bbox, intrinsic, joints_crop_img, joints_cam, heatmap, TrackTail{}, static_cast<hipStream_t>(stream)};
    return forward_ragged(h, fc, view_counts);
}

/* A camera-subset sweep (include/handmv.h): one backbone pass, the fusion tail per subset.  Everything that can be refused is refused, and
 * the whole call is planned on the host -- chunks, tables, workspace -- before the first launch.  Always eager. */
int hmv_forward_subsets(hmv_handle h, int32_t batch, int32_t n_subsets, const uint8_t *subset_mask, const float *x, const float *bbox,
                        const float *intrinsic, float *joints_crop_img, float *joints_cam, float *heatmap, void *stream) {
    if (const int rc = check_handle(h)) return rc;
    if (batch <= 0) return h->fail(HMV_ERR_ARG, "hmv_forward_subsets: batch must be positive (got %d)", (int)batch);
    if (n_subsets < 1) return h->fail(HMV_ERR_ARG, "hmv_forward_subsets: n_subsets must be at least 1 (got %d)", (int)n_subsets);
    if (!subset_mask) return h->fail(HMV_ERR_ARG, "hmv_forward_subsets: subset_mask is null (host uint8 [n_subsets][num_views])");
    if (!x || !joints_crop_img || !joints_cam) return h->fail(HMV_ERR_ARG, "hmv_forward_subsets: null or empty input/output");
    const int V = h->cfg.num_views, S = n_subsets;
    if ((long long)S * batch > INT32_MAX / (NJ * 3)) return h->fail(HMV_ERR_ARG, "hmv_forward_subsets: n_subsets x batch is too large");
    std::vector<int> count(S, 0);
    for (int i = 0; i < S; ++i) {
        for (int v = 0; v < V; ++v) count[i] += subset_mask[(size_t)i * V + v] != 0;
        if (!count[i]) return h->fail(HMV_ERR_ARG, "hmv_forward_subsets: subset %d has no camera", i);
    }
    const ForwardCall fc{batch, x, FrameSrc{}, bbox, intrinsic, joints_crop_img, joints_cam, heatmap, TrackTail{}, static_cast<hipStream_t>(stream)};
    // a subset's list is its cameras ascending
    std::vector<int> cams;
    cams.reserve((size_t)S * V);
    for (int i = 0; i < S; ++i)
        for (int v = 0; v < V; ++v)
            if (subset_mask[(size_t)i * V + v]) cams.push_back(v);
    return forward_camera_lists(h, fc, CameraLists{S, count, cams});
}

/* A reference-view sweep (include/handmv.h): hmv_forward_subsets with the cameras of every row fed in the order the row names them.
 * Everything that can be refused is refused before the first launch; the rest is hmv_forward_subsets' (one planner, one runner). */
int hmv_forward_orders(hmv_handle h, int32_t batch, int32_t n_orders, const int32_t *orders, const float *x, const float *bbox,
                       const float *intrinsic, float *joints_crop_img, float *joints_cam, float *heatmap, void *stream) {
    if (const int rc = check_handle(h)) return rc;
    if (batch <= 0) return h->fail(HMV_ERR_ARG, "hmv_forward_orders: batch must be positive (got %d)", (int)batch);
    if (n_orders < 1) return h->fail(HMV_ERR_ARG, "hmv_forward_orders: n_orders must be at least 1 (got %d)", (int)n_orders);
    if (!orders) return h->fail(HMV_ERR_ARG, "hmv_forward_orders: orders is null (host int32 [n_orders][num_views], padded with -1)");
    if (!x || !joints_crop_img || !joints_cam) return h->fail(HMV_ERR_ARG, "hmv_forward_orders: null or empty input/output");
    const int V = h->cfg.num_views, S = n_orders;
    if ((long long)S * batch > INT32_MAX / (NJ * 3)) return h->fail(HMV_ERR_ARG, "hmv_forward_orders: n_orders x batch is too large");
    std::vector<int> count(S, 0), cams;
    cams.reserve((size_t)S * V);
    std::vector<char> seen(V);
    for (int i = 0; i < S; ++i) {
        const int32_t *row = orders + (size_t)i * V;
        std::fill(seen.begin(), seen.end(), 0);
        for (int v = 0; v < V; ++v) {
            const int c = row[v];
            if (c < 0) {
                if (c != -1) return h->fail(HMV_ERR_ARG, "hmv_forward_orders: order %d, entry %d = %d is no camera in [0, %d) (padding is -1)", i, v, c, V);
                continue;
            }
            if (count[i] != v) return h->fail(HMV_ERR_ARG, "hmv_forward_orders: order %d names camera %d after a -1", i, c);
            if (c >= V) return h->fail(HMV_ERR_ARG, "hmv_forward_orders: order %d, entry %d = %d is no camera in [0, %d)", i, v, c, V);
            if (seen[c]) return h->fail(HMV_ERR_ARG, "hmv_forward_orders: order %d names camera %d twice", i, c);
            seen[c] = 1;
            cams.push_back(c);
            ++count[i];
        }
        if (!count[i]) return h->fail(HMV_ERR_ARG, "hmv_forward_orders: order %d has no camera", i);
    }
    const ForwardCall fc{batch, x, FrameSrc{}, bbox, intrinsic, joints_crop_img, joints_cam, heatmap, TrackTail{}, static_cast<hipStream_t>(stream)};
    return forward_camera_lists(h, fc, CameraLists{S, count, cams});
}

/* An occlusion sweep from raw frames (include/handmv.h): the per-frame stage once on the clean frames and once per occluded frame, the
 * fusion tail per variant.  Everything that can be refused is refused, and the whole call is planned on the host -- passes, tables,
 * workspace -- before the first launch.  Always eager. */
int hmv_forward_frames_occlusions(hmv_handle h, int32_t batch, const uint8_t *frames, int32_t frame_h, int32_t frame_w,
                                  const int32_t *crop_boxes, const float *mean, const float *std, const float *bbox, const float *intrinsic,
                                  int32_t n_occ, const int32_t *occ_view, const int32_t *occ_rects, float *joints_crop_img, float *joints_cam,
                                  float *heatmap, float *joints_crop_img_occ, float *heatmap_occ, void *stream) {
    if (const int rc = check_handle(h)) return rc;
    if (const int rc = check_frames(h, batch, frames, frame_h, frame_w, crop_boxes, mean, std, joints_crop_img, joints_cam)) return rc;
    if (n_occ < 1) return h->fail(HMV_ERR_ARG, "hmv_forward_frames_occlusions: n_occ must be at least 1 (got %d)", (int)n_occ);
    if (!occ_view) return h->fail(HMV_ERR_ARG, "hmv_forward_frames_occlusions: occ_view is null (host int32 [n_occ])");
    if (!occ_rects) return h->fail(HMV_ERR_ARG, "hmv_forward_frames_occlusions: occ_rects is null (device int32 [n_occ][batch][4])");
    const int V = h->cfg.num_views;
    if (((long long)n_occ + 1) * batch > INT32_MAX / (NJ * 3) / std::max(V, 1))   // (before occ_view's n_occ entries are read)
        return h->fail(HMV_ERR_ARG, "hmv_forward_frames_occlusions: (1 + n_occ) x batch is too large");
    for (int o = 0; o < n_occ; ++o)
        if (occ_view[o] < 0 || occ_view[o] >= V)
            return h->fail(HMV_ERR_ARG, "hmv_forward_frames_occlusions: occ_view[%d] = %d is no camera in [0, %d)", o, (int)occ_view[o], V);
    if (const int rc = check_crop_pe(h, bbox, intrinsic)) return rc;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    if (batch > h->reserved_batch)
        if (const int rc = hmv_reserve(h, batch)) return rc;
    // the passes: at most max(batch, reserved batch) * V occluded frames, then at most that many virtual samples each, so that every buffer
    // of a pass stays within the reservation
    const int cmax = std::max<int>(batch, h->reserved_batch), M = n_occ * batch, total = M + batch;
    OccPlan op;
    op.n_occ = n_occ;
    op.rects = occ_rects;
    op.crop_occ = joints_crop_img_occ;
    op.hm_occ = heatmap_occ;
    for (int q0 = 0; q0 < M; q0 += cmax * V) op.passes.push_back(OccPass{q0, std::min(cmax * V, M - q0)});
    ViewsUpload up{nullptr, (size_t)M};
    for (int q0 = 0; q0 < total; q0 += cmax) {
        const int nv = std::min(cmax, total - q0);
        op.chunks.push_back(SubsetChunk{q0, nv, nv * V, V, up.tab_n});
        up.tab_n += (size_t)nv + 1 + 2 * (size_t)nv * V;
    }
    if (const int rc = views_slot(h, up.tab_n, up.slot)) return rc;
    int32_t *index = up.slot->host;
    for (int q = 0; q < M; ++q) index[q] = (q % batch) * V + occ_view[q / batch];
    for (const SubsetChunk &ck : op.chunks) {
        int32_t *seg = up.slot->host + ck.tab, *fpos = seg + ck.nv + 1, *src = fpos + ck.n;
        seg[0] = 0;
        for (int i = 0, m = 0; i < ck.nv; ++i) {
            const int q = ck.q0 + i, o = q / batch - 1, b = q % batch;   // o == -1: the clean batch
            seg[i + 1] = seg[i] + NJ * V;
            for (int v = 0; v < V; ++v, ++m) {
                fpos[m] = NJ * v;
                src[m] = (o >= 0 && v == occ_view[o]) ? batch * V + o * batch + b : b * V + v;
            }
        }
    }
    const ForwardCall fc{batch, nullptr, frame_src(frames, frame_h, frame_w, crop_boxes, nullptr, 0, mean, std), bbox, intrinsic,
                         joints_crop_img, joints_cam, heatmap, TrackTail{}, static_cast<hipStream_t>(stream)};
    auto run = [&](const ForwardCall &c, bool dry, Arena &A) { return run_forward_occlusions(h, c, op, dry ? nullptr : h->views_dev, dry, A); };
    if (const int rc = plan_and_upload(h, fc, up, run)) return rc;
    h->forget_attention();   // (no attention maps: a sweep ignores the mask)
    return run_checked(h, fc, 1, run);
}

int hmv_op_prepare_frames_occluded(int32_t device, const uint8_t *frames, int32_t n_frames, int32_t frame_h, int32_t frame_w,
                                   const int32_t *crop_boxes, const int32_t *occ_rects, const float *mean, const float *std, int32_t out_h,
                                   int32_t out_w, float *out_nhwc4, void *stream) {
    if (!frames || !crop_boxes || !occ_rects || !mean || !std || !out_nhwc4 || n_frames <= 0 || frame_h <= 0 || frame_w <= 0 || out_h <= 0 ||
        out_w <= 0)
        return HMV_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return HMV_ERR_HIP;
    return launch_frames_to_input(frames, crop_boxes, n_frames, frame_h, frame_w, out_h, out_w, mean, std, 0, out_nhwc4,
                                  static_cast<hipStream_t>(stream), /*s2d=*/false, nullptr, 0, occ_rects) == hipSuccess ? HMV_OK : HMV_ERR_HIP;
}

int hmv_forward_frames_views(hmv_handle h, int32_t batch, const int32_t *view_counts, const uint8_t *frames, int32_t frame_h, int32_t frame_w,
                             const int32_t *crop_boxes, const int32_t *frame_index, const float *mean, const float *std, const float *bbox,
                             const float *intrinsic, float *joints_crop_img, float *joints_cam, float *heatmap, void *stream) {
    return forward_frames_views(h, batch, view_counts, frames, frame_h, frame_w, crop_boxes, frame_index, mean, std, bbox, intrinsic,
                                joints_crop_img, joints_cam, heatmap, TrackTail{}, stream);
}

int hmv_forward_frames(hmv_handle h, int32_t batch, const uint8_t *frames, int32_t frame_h, int32_t frame_w, const int32_t *crop_boxes,
                       const float *mean, const float *std, const float *bbox, const float *intrinsic, float *joints_crop_img,
                       float *joints_cam, float *heatmap, void *stream) {
    return forward_frames(h, batch, frames, frame_h, frame_w, crop_boxes, mean, std, bbox, intrinsic, joints_crop_img, joints_cam, heatmap,
                          TrackTail{}, stream);
}

/* hmv_forward_frames, then on the same stream the windows and bbox moved in place to the box around the joints just found
 * (include/handmv.h).  The tail is enqueued by the eager forward itself, so a captured graph holds it as its last node. */
int hmv_forward_frames_track(hmv_handle h, int32_t batch, const uint8_t *frames, int32_t frame_h, int32_t frame_w, int32_t *crop_boxes,
                             const float *mean, const float *std, float *bbox, const float *intrinsic, float *joints_crop_img,
                             float *joints_cam, float *heatmap, int32_t margin, int32_t square, float *joints_img, int32_t *status,
                             void *stream) {
    if (!h) return HMV_ERR_ARG;
    if (margin < 0) return h->fail(HMV_ERR_ARG, "hmv_forward_frames_track: margin must not be negative");
    return forward_frames(h, batch, frames, frame_h, frame_w, crop_boxes, mean, std, bbox, intrinsic, joints_crop_img, joints_cam, heatmap,
                          TrackTail{true, margin, square != 0, joints_img, status}, stream);
}

int hmv_forward_frames_views_track(hmv_handle h, int32_t batch, const int32_t *view_counts, const uint8_t *frames, int32_t frame_h,
                                   int32_t frame_w, int32_t *crop_boxes, const int32_t *frame_index, const float *mean, const float *std,
                                   float *bbox, const float *intrinsic, float *joints_crop_img, float *joints_cam, float *heatmap,
                                   int32_t margin, int32_t square, float *joints_img, int32_t *status, void *stream) {
    if (!h) return HMV_ERR_ARG;
    if (margin < 0) return h->fail(HMV_ERR_ARG, "hmv_forward_frames_views_track: margin must not be negative");
    return forward_frames_views(h, batch, view_counts, frames, frame_h, frame_w, crop_boxes, frame_index, mean, std, bbox, intrinsic,
                                joints_crop_img, joints_cam, heatmap, TrackTail{true, margin, square != 0, joints_img, status}, stream);
}

int hmv_op_prepare_frames(int32_t device, const uint8_t *frames, int32_t n_frames, int32_t frame_h, int32_t frame_w,
                          const int32_t *crop_boxes, const float *mean, const float *std, int32_t out_h, int32_t out_w, float *out_nhwc4,
                          void *stream) {
    if (!frames || !crop_boxes || !mean || !std || !out_nhwc4 || n_frames <= 0 || frame_h <= 0 || frame_w <= 0 || out_h <= 0 || out_w <= 0)
        return HMV_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return HMV_ERR_HIP;
    return launch_frames_to_input(frames, crop_boxes, n_frames, frame_h, frame_w, out_h, out_w, mean, std, 0, out_nhwc4,
                                  static_cast<hipStream_t>(stream)) == hipSuccess ? HMV_OK : HMV_ERR_HIP;
}

void hmv_destroy(hmv_handle h) {
    if (!h) return;
    (void)hipSetDevice(h->cfg.device);
    (void)hipDeviceSynchronize();
    h->drop_graphs();
    if (h->gstream) (void)hipStreamDestroy(h->gstream);
    if (h->aux) (void)hipStreamDestroy(h->aux);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    for (void *p : h->dev_allocs) (void)hipFree(p);
    if (h->sat) (void)hipFree(h->sat);
    if (h->views_dev) (void)hipFree(h->views_dev);
    for (auto &sl : h->views_host) {
        if (sl.host) (void)hipHostFree(sl.host);
        if (sl.done) (void)hipEventDestroy(sl.done);
    }
    if (h->arena) (void)hipFree(h->arena);
    for (float *p : {h->cap_feat0, h->cap_coords, h->cap_tokens, h->cap_fused})
        if (p) (void)hipFree(p);
    for (auto &m : h->att)
        for (float *p : {m.probs, m.share})
            if (p) (void)hipFree(p);
    for (auto &r : h->prof) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    delete h;
}

/* Test hook: fills the workspace arena with the byte `value` (0xFF = NaNs).  Every stage must write what a later stage reads:
 * a forward after poisoning must give the bits of a forward before it (tests/test_gpu_parity.py::test_poisoned_workspace). */
int hmv_poison_workspace(hmv_handle h, int32_t value, void *stream) {
    if (!h) return HMV_ERR_ARG;
    if (!h->arena || !h->arena_bytes) return HMV_OK;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipMemsetAsync(h->arena, value & 0xFF, h->arena_bytes, static_cast<hipStream_t>(stream)));
    return HMV_OK;
}

/* Fused tail kernels on (default) / off (the launch-per-op path they replace).  The choice is part of the workspace plan, so the
 * workspace is re-planned on the next forward. */
int hmv_set_tail_fusion(hmv_handle h, int32_t enable) {
    if (!h) return HMV_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipDeviceSynchronize());
    h->drop_graphs();
    h->ff_fuse = h->cheb_fuse = enable != 0;
    h->reserved_batch = 0;   // forces hmv_reserve to size the workspace again
    return HMV_OK;
}

/* Chained launches (Bottleneck conv3 -> the next block's conv1 from the output tile in LDS) on (default) / off (one launch per conv:
 * the same bits).  Part of the workspace plan, so the workspace is re-planned on the next forward. */
int hmv_set_chain_fusion(hmv_handle h, int32_t enable) {
    if (!h) return HMV_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipDeviceSynchronize());
    h->drop_graphs();
    h->chain_fuse = enable != 0;
    h->reserved_batch = 0;
    return HMV_OK;
}

int hmv_set_hr_fusion(hmv_handle h, int32_t enable) {
    if (!h) return HMV_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipDeviceSynchronize());
    h->drop_graphs();
    h->hr_fuse = (enable & 1) != 0;
    h->hr_overlap = (enable & 2) != 0;
    h->reserved_batch = 0;
    return HMV_OK;
}

int hmv_set_capture(hmv_handle h, int32_t enable) {
    if (!h) return HMV_ERR_ARG;
    h->capture = enable != 0;
    return HMV_OK;
}

int hmv_read_stage(hmv_handle h, const char *stage, float *dst, size_t capacity, void *stream) {
    if (!h || !stage || !dst) return HMV_ERR_ARG;
    const float *src = nullptr;
    size_t n = 0;
    const std::string st(stage);
    if (st == "feat0") { src = h->cap_feat0; n = h->cap_feat0_n; }
    else if (st == "coords_hm") { src = h->cap_coords; n = h->cap_coords_n; }
    else if (st == "tokens") { src = h->cap_tokens; n = h->cap_tokens_n; }
    else if (st == "fused") { src = h->cap_fused; n = h->cap_fused_n; }
    else return h->fail(HMV_ERR_ARG, "unknown stage %s", stage);
    if (h->last_ragged)
        return h->fail(HMV_ERR_STATE, "the last forward was a ragged one (hmv_forward_views): stages are captured by hmv_forward only");
    if (!src) return h->fail(HMV_ERR_STATE, "stage capture was not enabled before the forward");
    if (capacity < n) n = capacity;
    HIPCHK(h, hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    return HMV_OK;
}

/* Attention maps of the fusion blocks (include/handmv.h).  The buffers of an earlier mask stay until a forward under another non-zero one. */
int hmv_set_attention_capture(hmv_handle h, uint32_t block_mask) {
    if (!h) return HMV_ERR_ARG;
    const int nb = h->fusion_blocks();
    if (nb < 32 && (block_mask >> nb) != 0)
        return h->fail(HMV_ERR_ARG, "hmv_set_attention_capture: the mask 0x%x names a block at or above the %d fusion blocks of this model", (unsigned)block_mask, nb);
    h->att_mask = block_mask;   // (the buffers follow with the next forward or hmv_reserve: ensure_attention)
    return HMV_OK;
}

static int attention_block(hmv_handle h, const char *who, int32_t block, const hmv_engine::AttMap *&m) {
    if (block < 0 || block >= h->fusion_blocks())
        return h->fail(HMV_ERR_ARG, "%s: block %d is outside the %d fusion blocks of this model", who, (int)block, h->fusion_blocks());
    if (!((h->att_mask >> block) & 1u) || (size_t)block >= h->att.size() || !h->att[(size_t)block].valid)
        return h->fail(HMV_ERR_STATE, "%s: the last forward left no attention map of block %d (select it with hmv_set_attention_capture before "
                                      "the forward; a camera-subset sweep records none)", who, (int)block);
    m = &h->att[(size_t)block];
    return HMV_OK;
}

int hmv_attention_shape(hmv_handle h, int32_t block, int32_t *B, int32_t *Tq, int32_t *Tk, int32_t *views) {
    if (!h) return HMV_ERR_ARG;
    const hmv_engine::AttMap *m = nullptr;
    if (const int rc = attention_block(h, "hmv_attention_shape", block, m)) return rc;
    if (B) *B = m->B;
    if (Tq) *Tq = m->Tq;
    if (Tk) *Tk = m->Tk;
    if (views) *views = m->views;
    return HMV_OK;
}

int hmv_read_attention(hmv_handle h, int32_t block, float *probs, size_t probs_capacity, float *view_share, size_t share_capacity, void *stream) {
    if (!h) return HMV_ERR_ARG;
    const hmv_engine::AttMap *m = nullptr;
    if (const int rc = attention_block(h, "hmv_read_attention", block, m)) return rc;
    const size_t n = (size_t)m->B * 8 * m->Tq * m->Tk, ns = (size_t)m->B * 8 * m->Tq * m->views;
    if (view_share && !m->views)
        return h->fail(HMV_ERR_ARG, "hmv_read_attention: block %d lies behind the cross block, its 21 keys are no views: it has no view share", (int)block);
    if (probs && probs_capacity < n)
        return h->fail(HMV_ERR_ARG, "hmv_read_attention: the map of block %d holds %zu floats, probs_capacity is %zu", (int)block, n, probs_capacity);
    if (view_share && share_capacity < ns)
        return h->fail(HMV_ERR_ARG, "hmv_read_attention: the view share of block %d holds %zu floats, share_capacity is %zu", (int)block, ns, share_capacity);
    HIPCHK(h, hipSetDevice(h->cfg.device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (probs && n) HIPCHK(h, hipMemcpyAsync(probs, m->probs, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (view_share && ns) HIPCHK(h, hipMemcpyAsync(view_share, m->share, ns * sizeof(float), hipMemcpyDeviceToDevice, s));
    return HMV_OK;
}

int hmv_set_profiling(hmv_handle h, int32_t enable) {
    if (!h) return HMV_ERR_ARG;
    h->profiling = enable != 0;
    if (enable == 1) h->prof_used = 0;  // 1 starts a fresh record list, 0 pauses (records kept), 2 resumes; records accumulate
    return HMV_OK;
}

int hmv_profile_count(hmv_handle h) { return h ? (int)h->prof_used : 0; }

/* Device operations (kernel launches, memsets, device copies) the last eagerly run forward enqueued. */
int hmv_launch_count(hmv_handle h) { return h ? h->launches : 0; }

int hmv_range_status(hmv_handle h, int32_t *saturated, void *stream) {
    if (!h || !saturated) {
        if (h) h->fail(HMV_ERR_ARG, "hmv_range_status: null argument");
        return HMV_ERR_ARG;
    }
    *saturated = 0;
    HIPCHK(h, hipSetDevice(h->cfg.device));
    HIPCHK(h, hipStreamSynchronize(static_cast<hipStream_t>(stream)));   // (a second stream of the handle is joined into this one)
    int v = 0;
    HIPCHK(h, hipMemcpy(&v, h->sat, sizeof(int), hipMemcpyDeviceToHost));
    if (v) {
        const int zero = 0;
        HIPCHK(h, hipMemcpy(h->sat, &zero, sizeof(int), hipMemcpyHostToDevice));
    }
    *saturated = v != 0;
    return HMV_OK;
}

int hmv_profile_get(hmv_handle h, int32_t index, const char **name, const char **label, float *ms, double *flops) {
    if (!h || index < 0 || (size_t)index >= h->prof_used) return HMV_ERR_ARG;
    ProfRec &r = h->prof[index];
    float t = 0.f;
    HIPCHK(h, hipEventElapsedTime(&t, r.e0, r.e1));
    if (name) *name = r.name;
    if (label) *label = r.label.c_str();
    if (ms) *ms = t;
    if (flops) *flops = r.flops;
    return HMV_OK;
}

int hmv_profile_get_bytes(hmv_handle h, int32_t index, double *bytes) {
    if (!h || index < 0 || (size_t)index >= h->prof_used || !bytes) return HMV_ERR_ARG;
    *bytes = h->prof[index].bytes;
    return HMV_OK;
}

int hmv_op_attention(int32_t device, const float *qkv, int32_t B, int32_t T, int32_t Tq, int32_t koff, int32_t Tk, float *out,
                     void *stream) {
    if (!qkv || !out || B <= 0 || T <= 0 || Tq <= 0 || Tq > T || Tk <= 0 || koff < 0 || koff + Tk > T) {
        g_create_err = "hmv_op_attention: bad argument";
        return HMV_ERR_ARG;
    }
    if (hipSetDevice(device) != hipSuccess) { g_create_err = "hipSetDevice failed"; return HMV_ERR_HIP; }
    const hipError_t e = launch_attention(qkv, B, T, Tq, koff, Tk, out, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) { g_create_err = std::string("attention launch failed: ") + hipGetErrorString(e); return HMV_ERR_HIP; }
    return HMV_OK;
}

int hmv_op_attention_x3(int32_t device, const float *qkv, int32_t B, int32_t T, int32_t Tq, int32_t koff, int32_t Tk, float *out,
                        void *stream) {
    if (!qkv || !out || B <= 0 || T <= 0 || Tq <= 0 || Tq > T || Tk <= 0 || koff < 0 || koff + Tk > T) {
        g_create_err = "hmv_op_attention_x3: bad argument";
        return HMV_ERR_ARG;
    }
    if (hipSetDevice(device) != hipSuccess) { g_create_err = "hipSetDevice failed"; return HMV_ERR_HIP; }
    // the kernel takes rows of (hi, lo) fp16 pairs (what the projection GEMMs write in those modes): split the fp32 rows first
    hipStream_t s = static_cast<hipStream_t>(stream);
    void *pairs = nullptr;
    RangeWord rw;
    hipError_t e = rw.alloc();
    if (e == hipSuccess) e = op_guarded_alloc(&pairs, (size_t)B * T * 3072 * 4, s);
    if (e == hipSuccess) e = launch_rows_f32_to_half(qkv, pairs, (size_t)B * T, 3072, 2, s, rw.p);
    if (e == hipSuccess) e = launch_attention(static_cast<const float *>(pairs), B, T, Tq, koff, Tk, out, s, 0, 1, rw.p);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    op_guarded_free(pairs);
    if (e != hipSuccess) { g_create_err = std::string("attention launch failed: ") + hipGetErrorString(e); return HMV_ERR_HIP; }
    if (rw.saturated()) { g_create_err = "hmv_op_attention_x3: " + std::string(kRangeMsg); return HMV_ERR_RANGE; }
    return HMV_OK;
}

/* Test hook: the `pairs` epilogue of both attention bodies on its own (include/handmv.h). */
int hmv_op_attention_pairs(int32_t device, int32_t x3, const float *qkv, int32_t B, int32_t T, int32_t Tq, int32_t koff, int32_t Tk,
                           void *out_pairs, int32_t *sat, void *stream) {
    if (!qkv || !out_pairs || B <= 0 || T <= 0 || Tq <= 0 || Tq > T || Tk <= 0 || koff < 0 || koff + Tk > T || (x3 != 0 && x3 != 1)) {
        g_create_err = "hmv_op_attention_pairs: bad argument";
        return HMV_ERR_ARG;
    }
    if (hipSetDevice(device) != hipSuccess) { g_create_err = "hipSetDevice failed"; return HMV_ERR_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    float *out = static_cast<float *>(out_pairs);   // a row is 32 D bytes in either output form (AttSeg::rows)
    void *pairs = nullptr;
    RangeWord rw;
    hipError_t e = hipSuccess;
    if (x3) {   // the kernel takes rows of (hi, lo) fp16 pairs: split the fp32 rows first (hmv_op_attention_x3); the split reports to its own word
        e = rw.alloc();
        if (e == hipSuccess) e = op_guarded_alloc(&pairs, (size_t)B * T * 3072 * 4, s);
        if (e == hipSuccess) e = launch_rows_f32_to_half(qkv, pairs, (size_t)B * T, 3072, 2, s, rw.p);
        if (e == hipSuccess) e = launch_attention(static_cast<const float *>(pairs), B, T, Tq, koff, Tk, out, s, 1, 1, sat);
    } else {
        e = launch_attention(qkv, B, T, Tq, koff, Tk, out, s, 1, 0, sat);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    op_guarded_free(pairs);
    if (e != hipSuccess) { g_create_err = std::string("attention launch failed: ") + hipGetErrorString(e); return HMV_ERR_HIP; }
    if (x3 && rw.saturated()) { g_create_err = "hmv_op_attention_pairs: " + std::string(kRangeMsg); return HMV_ERR_RANGE; }
    return HMV_OK;
}

int hmv_op_attention_lq(int32_t device, const float *q, int32_t q_ld, int32_t q_bstride, const float *k, const float *v, int32_t kv_ld,
                        int32_t B, int32_t T, int32_t Tq, float *out, void *stream) {
    if (!q || !k || !v || !out || B <= 0 || T <= 0 || Tq <= 0 || q_ld < 2048 || kv_ld < 2048 || q_bstride < 0 || (q_ld & 3) || (kv_ld & 3)) {
        g_create_err = "hmv_op_attention_lq: bad argument";
        return HMV_ERR_ARG;
    }
    if (hipSetDevice(device) != hipSuccess) { g_create_err = "hipSetDevice failed"; return HMV_ERR_HIP; }
    const hipError_t e = launch_attention_d256(q, q_ld, q_bstride, k, v, kv_ld, B, T, Tq, out, static_cast<hipStream_t>(stream));
    if (e != hipSuccess) { g_create_err = std::string("attention launch failed: ") + hipGetErrorString(e); return HMV_ERR_HIP; }
    return HMV_OK;
}

/* Test hook: the ragged attention kernels on their own (include/handmv.h). */
int hmv_op_attention_views(int32_t device, int32_t kind, const float *qkv, const float *probe, int32_t B, const int32_t *seg_host, int32_t cross,
                           float *out, void *stream) {
    auto bad = [](const char *why) { g_create_err = std::string("hmv_op_attention_views: ") + why; return (int)HMV_ERR_ARG; };
    if (!qkv || !out || !seg_host || B <= 0 || kind < 0 || kind > 2) return bad("bad argument");
    if (kind == 2 && cross && !probe) return bad("the cross block of the 256-wide heads needs the probe queries");
    if (seg_host[0] != 0) return bad("seg[0] must be 0");
    int Tmax = 0;
    for (int b = 0; b < B; ++b) {
        const int T = seg_host[b + 1] - seg_host[b];
        if (T < 1 || (cross && kind != 2 && T < 21)) return bad("every sample needs at least one row, and 21 query rows in the cross block");
        Tmax = T > Tmax ? T : Tmax;
    }
    if (hipSetDevice(device) != hipSuccess) { g_create_err = "hipSetDevice failed"; return HMV_ERR_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t rows = (size_t)seg_host[B];
    int32_t *seg = nullptr;
    void *pairs = nullptr;
    RangeWord rw;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&seg), (size_t)(B + 1) * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpy(seg, seg_host, (size_t)(B + 1) * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && kind == 1) {   // the kernel takes rows of (hi, lo) fp16 pairs: split the fp32 rows first (hmv_op_attention_x3)
        e = rw.alloc();
        if (e == hipSuccess) e = op_guarded_alloc(&pairs, rows * 3072 * 4, s);
        if (e == hipSuccess) e = launch_rows_f32_to_half(qkv, pairs, rows, 3072, 2, s, rw.p);
        if (e == hipSuccess) e = launch_attention_views(static_cast<const float *>(pairs), B, seg, Tmax, cross, out, s, 0, 1, rw.p);
    } else if (e == hipSuccess && kind == 0) {
        e = launch_attention_views(qkv, B, seg, Tmax, cross, out, s);
    } else if (e == hipSuccess) {
        if (cross) e = launch_attention_d256_views(probe, 2048, 0, qkv, qkv + 2048, 4096, B, seg, Tmax, out, s);
        else e = launch_attention_d256_views(qkv, 6144, 1, qkv + 2048, qkv + 4096, 6144, B, seg, Tmax, out, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    op_guarded_free(pairs);
    if (seg) (void)hipFree(seg);
    if (e != hipSuccess) { g_create_err = std::string("attention launch failed: ") + hipGetErrorString(e); return HMV_ERR_HIP; }
    if (kind == 1 && rw.saturated()) { g_create_err = "hmv_op_attention_views: " + std::string(kRangeMsg); return HMV_ERR_RANGE; }
    return HMV_OK;
}

/* Test hook: the attention-map kernels on their own (include/handmv.h).  Every range is checked against the rows the caller describes
 * before anything is launched. */
int hmv_op_attention_probs(int32_t device, int32_t kind, const float *qkv, const float *probe, int32_t B, int32_t T, int32_t Tq, int32_t koff,
                           int32_t Tk, const int32_t *seg_host, float *probs, float *view_share, int32_t views, void *stream) {
    auto bad = [](const char *why) { g_create_err = std::string("hmv_op_attention_probs: ") + why; return (int)HMV_ERR_ARG; };
    if (!qkv || !probs || B <= 0 || kind < 0 || kind > 2) return bad("bad argument");
    if (probe && kind != 2) return bad("only the 256-wide heads (kind 2) take probe queries");
    if (koff < 0 || Tq < 0) return bad("koff and Tq must not be negative");
    if (probe && Tq <= 0) return bad("probe queries need their count Tq");
    int Tq_pad = Tq, Tk_pad = Tk;
    if (seg_host) {
        if (seg_host[0] != 0) return bad("seg[0] must be 0");
        int Tmax = 0;
        for (int b = 0; b < B; ++b) {
            const long long Tb = (long long)seg_host[b + 1] - seg_host[b];
            if (Tb < 1 || Tb > INT32_MAX / 2) return bad("every sample needs at least one row");
            if (Tb < koff) return bad("a sample has fewer rows than koff: its keys would start outside it");
            if (!probe && Tq > Tb) return bad("a sample has fewer rows than Tq: its queries would lie outside it");
            Tmax = (int)Tb > Tmax ? (int)Tb : Tmax;
        }
        Tq_pad = Tq ? Tq : Tmax;
        Tk_pad = Tmax - koff;
    } else {
        if (T <= 0 || Tq <= 0 || Tk <= 0) return bad("T, Tq and Tk must be positive");
        if (!probe && Tq > T) return bad("Tq > T: the queries would lie outside the sample");
        if ((long long)koff + Tk > T) return bad("koff + Tk > T: the keys would lie outside the sample");
        if ((long long)B * T > INT32_MAX / 2) return bad("B x T is too large");
    }
    if (view_share) {
        if (views <= 0 || koff % 21) return bad("a view share needs views > 0 and keys that start at a view (koff % 21 == 0)");
        for (int b = 0; b < B; ++b) {
            const int tk = seg_host ? seg_host[b + 1] - seg_host[b] - koff : Tk;
            if (tk % 21 || (koff + tk) / 21 > views) return bad("a view share needs key ranges of whole views (21 rows each), at most `views` of them");
        }
    }
    if (hipSetDevice(device) != hipSuccess) { g_create_err = "hipSetDevice failed"; return HMV_ERR_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t rows = seg_host ? (size_t)seg_host[B] : (size_t)B * T;
    int32_t *seg = nullptr;
    void *pairs = nullptr;
    RangeWord rw;
    hipError_t e = hipSuccess;
    if (seg_host) {
        e = hipMalloc(reinterpret_cast<void **>(&seg), (size_t)(B + 1) * sizeof(int32_t));
        if (e == hipSuccess) e = hipMemcpy(seg, seg_host, (size_t)(B + 1) * sizeof(int32_t), hipMemcpyHostToDevice);
    }
    // queries: the sample's own rows (q_seg / q_bstride = T), or the probe's, shared by every sample
    const AttnProbsRows pr = seg_host ? AttnProbsRows{seg, probe ? 0 : 1, koff, Tq, 0, 0, 0, 0, Tq_pad, Tk_pad}
                                      : AttnProbsRows{nullptr, 0, koff, 0, T, Tq, Tk, probe ? 0 : T, Tq_pad, Tk_pad};
    const size_t n = (size_t)B * 8 * Tq_pad * Tk_pad;
    if (e == hipSuccess && seg_host && n) e = hipMemsetAsync(probs, 0, n * sizeof(float), s);
    if (e == hipSuccess && n) {
        if (kind == 1) {   // the kernel takes rows of (hi, lo) fp16 pairs: split the fp32 rows first (hmv_op_attention_x3)
            e = rw.alloc();
            if (e == hipSuccess) e = op_guarded_alloc(&pairs, rows * 3072 * 4, s);
            if (e == hipSuccess) e = launch_rows_f32_to_half(qkv, pairs, rows, 3072, 2, s, rw.p);
            if (e == hipSuccess) e = launch_attention_probs(1, pairs, 6144, static_cast<const _Float16 *>(pairs) + 1024, 6144, B, pr, probs, s);
        } else if (kind == 0) {
            e = launch_attention_probs(0, qkv, 3072, qkv + 1024, 3072, B, pr, probs, s);
        } else if (probe) {
            e = launch_attention_probs(2, probe, 2048, qkv, 4096, B, pr, probs, s);
        } else {
            e = launch_attention_probs(2, qkv, 6144, qkv + 2048, 6144, B, pr, probs, s);
        }
    }
    if (e == hipSuccess && view_share) {
        const size_t ns = (size_t)B * 8 * Tq_pad * views;
        if (n) e = launch_attention_share(probs, B, pr, koff / 21, views, view_share, s);
        else e = hipMemsetAsync(view_share, 0, ns * sizeof(float), s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    op_guarded_free(pairs);
    if (seg) (void)hipFree(seg);
    if (e != hipSuccess) { g_create_err = std::string("attention map launch failed: ") + hipGetErrorString(e); return HMV_ERR_HIP; }
    if (kind == 1 && rw.saturated()) { g_create_err = "hmv_op_attention_probs: " + std::string(kRangeMsg); return HMV_ERR_RANGE; }
    return HMV_OK;
}

}  // extern "C"

// One conv through the engine's own packing (Loader::conv) and launch path (Runner::conv) under `route`: what every hmv_op_conv2d*
// entry runs.  HMV_F32 reads and writes fp32 rows; HMV_F16 / HMV_F32X3 convert the input (and residual) rows first, and with out16
// the layer writes fp16 rows, as every backbone layer of the fp16 path does.  tall: conv_ht.hip's K order.  rd: the row-decomposed
// packing of a 3x3 C -> C conv, whose bias is then the shift of an identity BatchNorm (that packing takes its shift from one).
static int op_conv(const char *who, int32_t device, int32_t dtype, const float *in, int32_t N, int32_t H, int32_t W, int32_t Cin,
                   const float *w_oihw, const float *bias_host, int32_t Cout, int32_t R, int32_t S, int32_t stride, int32_t pad,
                   const float *residual, int32_t relu, void *out, bool out16, const ConvRoute &route, const char **kernel_name,
                   void *stream, bool tall = false, bool rd = false, int Ho_cut = 0, int Wo_cut = 0) {
    if (tall && (residual || !out16 || !conv_ht_shape_ok(R, S, stride, pad, Cin, Cout, H, W))) {
        g_create_err = std::string(who) + ": the tall-tile kernel takes 3x3 stride-1 pad-1 convs without residual, Cin % 32 == 0 (>= 64), Cout % 128 == 0, H % 16 == 0, W % 32 == 0";
        return HMV_ERR_ARG;
    }
    const bool half = dtype != HMV_F32;
    if ((half && dtype != HMV_F16 && dtype != HMV_F32X3) || !in || !w_oihw || !out || Cin % (half ? 8 : 4) != 0 || (half && Cout % 4 != 0) ||
        (out16 && dtype != HMV_F16)) {
        g_create_err = std::string(who) + ": dtype must be HMV_F32 / HMV_F16 / HMV_F32X3; fp32 needs Cin % 4 == 0, the fp16-based modes Cin % 8 == 0, Cout % 4 == 0";
        return HMV_ERR_ARG;
    }
    if (hipSetDevice(device) != hipSuccess) { g_create_err = "hipSetDevice failed"; return HMV_ERR_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    hmv_engine eng;
    eng.cfg.device = device;
    HostTensor wt, bt;
    wt.shape = {Cout, Cin, R, S};
    wt.data.assign(w_oihw, w_oihw + (size_t)Cout * Cin * R * S);
    eng.host["w"] = wt;
    bt.shape = {Cout};
    bt.data.assign(Cout, 0.f);
    if (bias_host) bt.data.assign(bias_host, bias_host + Cout);
    if (rd) {
        HostTensor g1 = bt, m0 = bt, v1 = bt;
        g1.data.assign(Cout, 1.f); m0.data.assign(Cout, 0.f);
        v1.data.assign(Cout, 1.f - 1e-5f);   // scale = 1 / sqrt(var + eps) == 1 to fp32 rounding
        eng.host["bn.weight"] = g1; eng.host["bn.bias"] = bt; eng.host["bn.running_mean"] = m0; eng.host["bn.running_var"] = v1;
    } else if (bias_host) {
        eng.host["b"] = bt;
    }
    Loader L{&eng};
    L.split = dtype == HMV_F32X3;
    Layer layer;
    L.conv(layer, "op", "w", bias_host && !rd ? "b" : "", rd ? "bn" : "", Cout, Cin, R, S, 0, half, rd, nullptr, tall);
    int rc = L.rc;
    if (rc == HMV_OK && rd && !layer.rd_cout) { eng.err = "the layer was not packed row-decomposed"; rc = HMV_ERR_ARG; }
    int Ho = (H + 2 * pad - R) / stride + 1, Wo = (W + 2 * pad - S) / stride + 1;
    if (Ho_cut > 0 && Ho_cut <= Ho) Ho = Ho_cut;   // (hmv_op_conv2d_as: the top-left Ho x Wo of the conv's map, residual and output rows of that size)
    if (Wo_cut > 0 && Wo_cut <= Wo) Wo = Wo_cut;
    const void *x = in, *res = residual;
    void *din = nullptr, *dres = nullptr;
    RangeWord rw;
    hipError_t e = rc == HMV_OK ? rw.alloc() : hipSuccess;
    eng.sat = rw.p;
    if (rc == HMV_OK && e == hipSuccess && half) {   // fp16 rows, or (hi, lo) pairs in HMV_F32X3
        const int mode = dtype == HMV_F32X3 ? 2 : 1;
        const size_t rows_in = (size_t)N * H * W, rows_out = (size_t)N * Ho * Wo;
        e = op_guarded_alloc(&din, rows_in * Cin * 2 * mode, s);
        if (e == hipSuccess && residual) e = op_guarded_alloc(&dres, rows_out * Cout * 2 * mode, s);
        if (e == hipSuccess) e = launch_rows_f32_to_half(in, din, rows_in, Cin, mode, s, rw.p);
        if (e == hipSuccess && residual) e = launch_rows_f32_to_half(residual, dres, rows_out, Cout, mode, s, rw.p);
        x = din;
        res = dres;
    }
    if (rc == HMV_OK && e == hipSuccess) {
        Arena dummy;
        Runner Rn{&eng, s, false, HMV_OK, dummy};
        Rn.kernel_name = kernel_name;
        Rn.route = route;
        Rn.conv(ConvCall(layer, static_cast<const float *>(x), N, H, W, static_cast<float *>(out), Cout, Ho, Wo).s(stride).pad(pad)
                    .add(static_cast<const float *>(res), Cout).act(relu ? ACT_RELU : ACT_NONE).f16(out16));
        rc = Rn.rc;
        if (rc == HMV_OK) e = hipStreamSynchronize(s);
    }
    op_guarded_free(din);
    op_guarded_free(dres);
    for (void *ptr : eng.dev_allocs) (void)hipFree(ptr);
    if (rc != HMV_OK) { g_create_err = std::string(who) + ": " + eng.err; return rc; }
    if (e != hipSuccess) { g_create_err = std::string(who) + ": " + hipGetErrorString(e); return HMV_ERR_HIP; }
    if (rw.saturated()) { g_create_err = std::string(who) + ": " + kRangeMsg; return HMV_ERR_RANGE; }
    return HMV_OK;
}

// kernel_sel -> route of the op-level entries (include/handmv.h).  Families a sel does not name keep the launcher's rule.
static ConvRoute route_sel(int sel) {   // hmv_op_conv2d_sel: 1 conv_igemm, 2 conv_stream_f32 whenever the shape has an instantiation
    ConvRoute r = conv_rule();
    if (sel) r.stream = sel == 2 ? ROUTE_FORCE : ROUTE_NEVER;
    return r;
}
static ConvRoute route_f16(int sel) {
    ConvRoute r = conv_rule();
    if (sel) r.stream = r.gemm8 = r.hs = (sel == 2 || sel == 8) ? ROUTE_FORCE : ROUTE_NEVER;   // (3 .. 7 keep the other special kernels out)
    if (sel >= 3 && sel <= 7) r.ht = (sel == 4 || sel == 6) ? ROUTE_NEVER : ROUTE_FORCE;
    r.ht_m16 = sel != 5 && sel != 6;
    r.ht_persist = sel == 7 ? 2 : (sel == 3 ? 0 : 1);
    r.gemm8_persist = sel == 8 ? 2 : (sel == 2 ? 0 : 1);
    return r;
}
static ConvRoute route_x3(int sel) {   // hmv_op_conv2d_x3: 1 conv_igemm's fused split loop, 2 gemm_x3k16 whenever the shape allows
    ConvRoute r = conv_rule();
    if (sel) r.x3k16 = sel == 2 ? ROUTE_FORCE : ROUTE_NEVER;
    return r;
}
static ConvRoute route_rd(int sel) {   // hmv_op_conv2d_rd: 1 conv_igemm's row-decomposed tiles, 2 conv_rds whatever the size
    ConvRoute r = conv_rule();
    if (sel) r.rds = sel == 2 ? ROUTE_FORCE : ROUTE_NEVER;
    return r;
}

extern "C" {

int hmv_op_conv2d(int32_t device, const float *in, int32_t N, int32_t H, int32_t W, int32_t Cin, const float *w_oihw,
                  const float *bias_host, int32_t Cout, int32_t R, int32_t S, int32_t stride, int32_t pad, const float *residual,
                  int32_t relu, float *out, void *stream) {
    return op_conv("hmv_op_conv2d", device, HMV_F32, in, N, H, W, Cin, w_oihw, bias_host, Cout, R, S, stride, pad, residual, relu, out, false,
                   conv_rule(), nullptr, stream);
}

int hmv_op_conv2d_ex(int32_t device, int32_t dtype, const float *in, int32_t N, int32_t H, int32_t W, int32_t Cin, const float *w_oihw,
                     const float *bias_host, int32_t Cout, int32_t R, int32_t S, int32_t stride, int32_t pad, const float *residual,
                     int32_t relu, float *out, void *stream) {
    return op_conv("hmv_op_conv2d_ex", device, dtype, in, N, H, W, Cin, w_oihw, bias_host, Cout, R, S, stride, pad, residual, relu, out, false,
                   conv_rule(), nullptr, stream);
}

int hmv_op_conv2d_sel(int32_t device, const float *in, int32_t N, int32_t H, int32_t W, int32_t Cin, const float *w_oihw, const float *bias_host,
                      int32_t Cout, int32_t R, int32_t S, int32_t stride, int32_t pad, const float *residual, int32_t relu, float *out,
                      int32_t kernel_sel, const char **kernel_name, void *stream) {
    if (kernel_sel < 0 || kernel_sel > 2) { g_create_err = "hmv_op_conv2d_sel: kernel_sel must be 0, 1 or 2"; return HMV_ERR_ARG; }
    return op_conv("hmv_op_conv2d_sel", device, HMV_F32, in, N, H, W, Cin, w_oihw, bias_host, Cout, R, S, stride, pad, residual, relu, out, false,
                   route_sel(kernel_sel), kernel_name, stream);
}

int hmv_op_conv2d_f16(int32_t device, const float *in, int32_t N, int32_t H, int32_t W, int32_t Cin, const float *w_oihw, const float *bias_host,
                      int32_t Cout, int32_t R, int32_t S, int32_t stride, int32_t pad, const float *residual, int32_t relu, void *out_f16,
                      int32_t kernel_sel, const char **kernel_name, void *stream) {
    if (kernel_sel < 0 || kernel_sel > 8) { g_create_err = "hmv_op_conv2d_f16: kernel_sel must be 0 .. 8"; return HMV_ERR_ARG; }
    return op_conv("hmv_op_conv2d_f16", device, HMV_F16, in, N, H, W, Cin, w_oihw, bias_host, Cout, R, S, stride, pad, residual, relu, out_f16,
                   true, route_f16(kernel_sel), kernel_name, stream, kernel_sel >= 3 && kernel_sel <= 7);   // (3 .. 7: the tall-tile packing)
}

int hmv_op_conv2d_x3(int32_t device, const float *in, int32_t N, int32_t H, int32_t W, int32_t Cin, const float *w_oihw, const float *bias_host,
                     int32_t Cout, int32_t R, int32_t S, int32_t stride, int32_t pad, const float *residual, int32_t relu, float *out,
                     int32_t kernel_sel, const char **kernel_name, void *stream) {
    if (kernel_sel < 0 || kernel_sel > 2) { g_create_err = "hmv_op_conv2d_x3: kernel_sel must be 0, 1 or 2"; return HMV_ERR_ARG; }
    return op_conv("hmv_op_conv2d_x3", device, HMV_F32X3, in, N, H, W, Cin, w_oihw, bias_host, Cout, R, S, stride, pad, residual, relu, out, false,
                   route_x3(kernel_sel), kernel_name, stream);
}

// One fp32 3x3 stride-1 pad-1 conv C -> C in the ROW-DECOMPOSED packing: what HRNet-w40's 40- / 80-channel branches run
int hmv_op_conv2d_rd(int32_t device, const float *in, int32_t N, int32_t H, int32_t W, int32_t C, const float *w_oihw, const float *bias_host,
                     const float *residual, int32_t relu, float *out, int32_t kernel_sel, const char **kernel_name, void *stream) {
    if (!in || !w_oihw || !out || C % 4 != 0 || 3 * C > 256 || C % 32 == 0 || W <= 0 || 128 % W != 0 || kernel_sel < 0 || kernel_sel > 2) {
        g_create_err = "hmv_op_conv2d_rd: C % 4 == 0, C % 32 != 0, 3 C <= 256, 128 % W == 0, kernel_sel 0 .. 2";
        return HMV_ERR_ARG;
    }
    return op_conv("hmv_op_conv2d_rd", device, HMV_F32, in, N, H, W, C, w_oihw, bias_host, C, 3, 3, 1, 1, residual, relu, out, false,
                   route_rd(kernel_sel), kernel_name, stream, false, true);
}

int hmv_op_conv2d_as(int32_t device, int32_t dtype, const float *in, int32_t N, int32_t H, int32_t W, int32_t Cin, const float *w_oihw,
                     const float *bias_host, int32_t Cout, int32_t R, int32_t S, int32_t stride, int32_t pad, const float *residual,
                     int32_t relu, float *out, int32_t Ho, int32_t Wo, int32_t packing, const char **kernel_name, void *stream) {
    const int Ho_own = (H + 2 * pad - R) / stride + 1, Wo_own = (W + 2 * pad - S) / stride + 1;
    const bool rd = packing == 1;
    if (packing < 0 || packing > 1 || Ho < 0 || Wo < 0 || Ho > Ho_own || Wo > Wo_own ||
        (rd && (dtype != HMV_F32 || R != 3 || S != 3 || stride != 1 || pad != 1 || Ho || Wo || Cout % 4 != 0 || 3 * Cout > 256 || W <= 0 || 128 % W != 0))) {
        g_create_err = "hmv_op_conv2d_as: packing 0 / 1 (1: fp32 3x3 stride 1 pad 1, Cout % 4 == 0, 3 Cout <= 256, 128 % W == 0, own map size), Ho x Wo within the conv's own map";
        return HMV_ERR_ARG;
    }
    return op_conv("hmv_op_conv2d_as", device, dtype, in, N, H, W, Cin, w_oihw, bias_host, Cout, R, S, stride, pad, residual, relu, out, false,
                   conv_rule(), kernel_name, stream, false, rd, Ho, Wo);
}

// One launch in a form that only a forward issues otherwise (include/handmv.h): the loader's packing (Loader::conv, conv_dual,
// deconv_phases / deconv_merge), the Runner's launch path (conv, conv_slices, chains_into), guarded temporaries as in op_conv.  What the
// engine would never issue is refused by the rules the engine itself asks (chains_into, conv_hs_supported, splitk_slices, launch_conv)
int hmv_op_conv2d_form(int32_t device, hmv_conv_form_args *a, void *stream) {
    static const char *who = "hmv_op_conv2d_form";
    auto bad = [&](const std::string &why) { g_create_err = std::string(who) + ": " + why; return (int)HMV_ERR_ARG; };
    if (!a) return bad("args is NULL");
    if (a->struct_size != (int32_t)sizeof(hmv_conv_form_args)) return bad("struct_size does not match this library's hmv_conv_form_args");
    a->kernel_name = nullptr;
    const int form = a->form, dtype = a->dtype;
    const bool dual = form & HMV_FORM_DUAL, chain = form & HMV_FORM_CHAIN, pool = form & HMV_FORM_POOL, phases = form & HMV_FORM_PHASES,
               splitk = form & HMV_FORM_SPLITK, pair_out = form & HMV_FORM_PAIR_OUT;
    if (form & ~63) return bad("form holds an unknown bit");
    if (dtype != HMV_F32 && dtype != HMV_F16 && dtype != HMV_F32X3) return bad("dtype must be HMV_F32, HMV_F16 or HMV_F32X3");
    const bool half = dtype != HMV_F32, x3 = dtype == HMV_F32X3;
    if (!a->in || !a->w || !a->out || a->N <= 0 || a->H <= 0 || a->W <= 0 || a->Cin <= 0 || a->Cout <= 0 || a->R <= 0 || a->S <= 0 ||
        a->stride <= 0 || a->pad < 0)
        return bad("null operand or non-positive size");
    if ((long long)a->N * a->H * a->W > INT32_MAX / 8) return bad("N x H x W is too large");
    if ((int)pool + (int)phases + (int)splitk + (int)(dual || chain) > 1) return bad("pool, phases, split-K and dual / chain do not meet in one launch");
    if (pair_out && (!x3 || dual || chain || pool || splitk))
        return bad("the pair-output epilogue belongs to HMV_F32X3 layers (plain or phases)");
    if ((chain || pool) && dtype != HMV_F16) return bad("chain and pool are forms of HMV_F16");
    if (splitk && dtype != HMV_F32) return bad("split-K is a form of HMV_F32");
    if (dual && x3) return bad("the pair mode runs conv3 and downsample as two launches");
    const int unit = half ? 8 : 4;
    const int Cin = a->Cin, Cout = a->Cout;
    const int ld_in = a->ld_in ? a->ld_in : Cin, ldc = a->ldc ? a->ldc : Cout, ldr = a->ldr ? a->ldr : Cout;
    if (ld_in < Cin || ld_in % unit || ldc < Cout || ldc % 4 || (a->residual && (ldr < Cout || ldr % unit)) || (half && Cout % 4))
        return bad("row strides: ld_in >= Cin, ldc >= Cout, ldr >= Cout, whole 16-byte units of the mode's storage (fp32 4, fp16-based 8 elements; ldc 4)");
    int Ho = 0, Wo = 0, Hout = 0, Wout = 0;   // launch grid; rows of `out`
    if (phases) {
        if (a->R != 4 || a->S != 4 || a->stride != 2 || a->pad != 1 || a->residual || a->Ho || a->Wo || ld_in != Cin)
            return bad("phases: a ConvTranspose2d(4, 2, 1) without residual (R = S = 4, stride 2, pad 1), dense input rows, its own map size");
        if (Cin % (half ? 64 : 32)) return bad("phases: whole 32 (fp32) / 64 (fp16) channel chunks");
        if (a->merged != 0 && a->merged != 1) return bad("merged must be 0 or 1");
        if (a->merged && x3) return bad("the pair mode issues the four phase launches only");
        if (x3 != pair_out) return bad("phases in HMV_F32X3 write pairs, as the engine's do");
        Ho = a->H; Wo = a->W; Hout = 2 * a->H; Wout = 2 * a->W;
    } else {
        const int Ho_own = (a->H + 2 * a->pad - a->R) / a->stride + 1, Wo_own = (a->W + 2 * a->pad - a->S) / a->stride + 1;
        if (Ho_own <= 0 || Wo_own <= 0 || a->Ho < 0 || a->Wo < 0 || a->Ho > Ho_own || a->Wo > Wo_own) return bad("Ho x Wo within the conv's own map");
        Ho = a->Ho ? a->Ho : Ho_own; Wo = a->Wo ? a->Wo : Wo_own;
        Hout = Ho; Wout = Wo;
    }
    if (dual) {
        if (!a->in2 || !a->w2 || a->Cin2 <= 0 || a->H2 <= 0 || a->W2 <= 0 || a->stride2 <= 0) return bad("dual: in2, w2, Cin2, H2, W2, stride2");
        const int ld2 = a->ld_in2 ? a->ld_in2 : a->Cin2;
        if (a->R != 1 || a->S != 1 || a->stride != 1 || a->pad || a->residual || ld_in != Cin || ld2 < a->Cin2 || ld2 % unit)
            return bad("dual: a 1x1 stride-1 conv without residual, ld_in = Cin, ld_in2 >= Cin2 in whole 16-byte units");
        if ((long long)(Ho - 1) * a->stride2 > a->H2 - 1 || (long long)(Wo - 1) * a->stride2 > a->W2 - 1)
            return bad("dual: the sampled pixels (ho * stride2, wo * stride2) lie outside the H2 x W2 map");
    }
    if (chain && (!a->next_w || !a->next_out || a->next_cout <= 0 || a->next_cout % 8)) return bad("chain: next_w, next_out, next_cout in whole 16-byte rows");
    if (pool && (a->pool_h <= 0 || a->pool_w <= 0 || a->residual)) return bad("pool: pool_h, pool_w, no residual");
    if (splitk && (a->slices < 1 || a->R != 1 || a->S != 1 || a->H != 1 || a->W != 1 || a->stride != 1 || a->pad || a->residual || a->relu || ld_in != Cin))
        return bad("split-K: GEMM rows (H = W = 1, 1x1), slices >= 1, no residual, no activation");
    auto rt = [&](int v, int &dst) { if (v == 1) dst = ROUTE_NEVER; else if (v == 2) dst = ROUTE_FORCE; return v >= 0 && v <= 2; };
    ConvRoute route = conv_rule();
    if (!rt(a->route_stream, route.stream) || !rt(a->route_gemm8, route.gemm8) || !rt(a->route_hs, route.hs) || !rt(a->route_x3k16, route.x3k16) ||
        a->gemm8_persist < 0 || a->gemm8_persist > 2)
        return bad("route_* and gemm8_persist must be 0 (the rule), 1 (never) or 2 (forced / wherever it exists)");
    if (a->gemm8_persist) route.gemm8_persist = a->gemm8_persist == 2 ? 2 : 0;
    if (hipSetDevice(device) != hipSuccess) { g_create_err = "hipSetDevice failed"; return HMV_ERR_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream);

    // ---- packing: the loader's
    hmv_engine eng;
    eng.cfg.device = device;
    eng.cfg.dtype = dtype;
    Loader L{&eng};
    L.split = x3;
    Layer layer, next, dl[4], dall;
    size_t dstride = 0;
    const std::vector<double> one(Cout, 1.0), zero(Cout, 0.0);
    std::vector<float> b1(Cout, 0.f);
    if (a->bias) b1.assign(a->bias, a->bias + Cout);
    if (phases) {
        L.deconv_phases(dl, "op", a->w, b1.data(), Cin, Cout, one, zero, half);
        if (a->merged) {
            L.deconv_merge(dl, dall, dstride, "op", half);
            if (L.rc == HMV_OK && !dall.w) { eng.err = "the merged phase layer was not made"; L.rc = HMV_ERR_ARG; }
        }
    } else if (dual) {
        std::vector<double> bd1(b1.begin(), b1.end()), bd2(Cout, 0.0);
        if (a->bias2) bd2.assign(a->bias2, a->bias2 + Cout);
        if (!L.conv_dual(layer, "op+downsample", a->w, a->w2, Cin, a->Cin2, Cout, one, bd1, one, bd2, half))
            return bad("dual: whole 32 (fp32) / 64 (fp16) channel chunks on either side of the seam");
    } else {
        HostTensor wt, bt;
        wt.shape = {Cout, Cin, a->R, a->S};
        wt.data.assign(a->w, a->w + (size_t)Cout * Cin * a->R * a->S);
        eng.host["w"] = wt;
        bt.shape = {Cout};
        bt.data = b1;
        if (a->bias) eng.host["b"] = bt;
        L.conv(layer, "op", "w", a->bias ? "b" : "", "", Cout, Cin, a->R, a->S, ld_in != Cin ? ld_in : 0, half);
    }
    if (chain) {
        HostTensor wt, bt;
        wt.shape = {a->next_cout, Cout, 1, 1};
        wt.data.assign(a->next_w, a->next_w + (size_t)a->next_cout * Cout);
        eng.host["nw"] = wt;
        bt.shape = {a->next_cout};
        bt.data.assign(a->next_cout, 0.f);
        if (a->next_bias) bt.data.assign(a->next_bias, a->next_bias + a->next_cout);
        eng.host["nb"] = bt;
        L.conv(next, "next", "nw", "nb", "", a->next_cout, Cout, 1, 1, 0, true);
    }
    if (splitk) eng.zero_bias = L.upload(std::vector<float>(4096, 0.f));
    int rc = L.rc;

    // ---- operands in the mode's storage format
    const size_t rows_in = (size_t)a->N * a->H * a->W, rows_out = (size_t)a->N * Hout * Wout;
    const void *x = a->in, *res = a->residual, *x2 = a->in2;
    void *din = nullptr, *dres = nullptr, *din2 = nullptr;
    const int ld2 = dual ? (a->ld_in2 ? a->ld_in2 : a->Cin2) : 0;
    RangeWord rw;
    hipError_t e = rc == HMV_OK ? rw.alloc() : hipSuccess;
    eng.sat = rw.p;
    if (rc == HMV_OK && e == hipSuccess && half) {
        const int mode = x3 ? 2 : 1;
        e = op_guarded_alloc(&din, rows_in * ld_in * 2 * mode, s);
        if (e == hipSuccess) e = launch_rows_f32_to_half(a->in, din, rows_in, ld_in, mode, s, rw.p);
        x = din;
        if (e == hipSuccess && a->residual) {
            e = op_guarded_alloc(&dres, rows_out * ldr * 2 * mode, s);
            if (e == hipSuccess) e = launch_rows_f32_to_half(a->residual, dres, rows_out, ldr, mode, s, rw.p);
            res = dres;
        }
        if (e == hipSuccess && dual) {
            const size_t rows2 = (size_t)a->N * a->H2 * a->W2;
            e = op_guarded_alloc(&din2, rows2 * ld2 * 2, s);
            if (e == hipSuccess) e = launch_rows_f32_to_half(a->in2, din2, rows2, ld2, 1, s, rw.p);
            x2 = din2;
        }
    }

    // ---- the launch(es): the Runner's
    const char *kname = nullptr;
    if (rc == HMV_OK && e == hipSuccess) {
        Arena dummy;
        Runner Rn{&eng, s, false, HMV_OK, dummy};
        Rn.kernel_name = &kname;
        Rn.route = route;
        const float *xf = static_cast<const float *>(x);
        float *of = static_cast<float *>(a->out);
        const int act = a->relu ? ACT_RELU : ACT_NONE;
        const bool out16 = dtype == HMV_F16 || pair_out;
        if (phases) {
            if (a->merged)
                Rn.conv(ConvCall(dall, xf, a->N, a->H, a->W, of, ldc, Ho, Wo).pad(1).act(act).f16(out16).all_phases(4, dstride));
            else
                for (int pa = 0; pa < 2; ++pa)
                    for (int pb = 0; pb < 2; ++pb)
                        Rn.conv(ConvCall(dl[pa * 2 + pb], xf, a->N, a->H, a->W, of, ldc, Ho, Wo).pad(1 - pa, 1 - pb).act(act).f16(out16).phase(pa, pb));
        } else if (splitk) {
            const int rule = Runner::splitk_slices(layer, a->N);
            if (a->slices != 1 && a->slices != rule) {
                eng.err = "the engine cuts this layer into " + std::to_string(rule) + " slice(s), or runs it whole";
                Rn.rc = HMV_ERR_ARG;
            } else {
                Rn.conv_slices(layer, xf, a->N, a->slices, of, ldc);
            }
        } else {
            ConvCall c(layer, xf, a->N, a->H, a->W, of, ldc, Ho, Wo);
            c.s(a->stride).pad(a->pad).add(static_cast<const float *>(res), ldr).act(act).f16(out16);
            if (dual) c.second(static_cast<const float *>(x2), Cin, a->H2, a->W2, ld2, a->stride2);
            if (chain) {
                Block nb;
                nb.c1 = next;
                if (!Rn.chains_into(c, &nb)) { eng.err = "the engine does not chain this launch into a 1x1 conv of next_cout channels"; Rn.rc = HMV_ERR_ARG; }
                c.chain(next, static_cast<float *>(a->next_out));
            }
            if (pool) {
                c.pooled(a->pool_h, a->pool_w);
                if (!conv_hs_supported(Rn.params(c), route)) { eng.err = "the engine does not pool behind this launch (conv_hs_supported)"; Rn.rc = HMV_ERR_ARG; }
            }
            Rn.conv(c);
        }
        rc = Rn.rc;
        if (rc == HMV_OK) e = hipStreamSynchronize(s);
    }
    op_guarded_free(din);
    op_guarded_free(dres);
    op_guarded_free(din2);
    for (void *ptr : eng.dev_allocs) (void)hipFree(ptr);
    if (rc != HMV_OK) { g_create_err = std::string(who) + ": " + eng.err; return rc; }
    if (e != hipSuccess) { g_create_err = std::string(who) + ": " + hipGetErrorString(e); return HMV_ERR_HIP; }
    a->kernel_name = kname;
    if (rw.saturated()) { g_create_err = std::string(who) + ": " + kRangeMsg; return HMV_ERR_RANGE; }
    return HMV_OK;
}

}  // extern "C"

// The up-sampling terms of an HRNet fuse layer through hr_fuse.hip alone (op-level parity tests): out = act(base + sum_s up_{2^shift_s}(W_s x_s + b_s)),
// terms added in the order given.  base / x_s device fp32 NHWC; f16 != 0 runs the fp16 instantiation on fp16 copies of them and `out` receives
// fp16 rows (else fp32).  Weights [C][C_s] and biases [C] on the host.
extern "C" int hmv_op_hr_fuse_up(int32_t device, int32_t f16, const float *base, int32_t N, int32_t H, int32_t W, int32_t C, int32_t nsrc,
                                 const float *const *src, const int32_t *src_c, const int32_t *shift, const float *const *w_host,
                                 const float *const *bias_host, int32_t relu, void *out, void *stream) {
    if (!base || !out || !src || !src_c || !shift || !w_host || !bias_host || nsrc < 1 || nsrc > 3 || N <= 0 || H <= 0 || W <= 0 || C <= 0) {
        g_create_err = "hmv_op_hr_fuse_up: bad arguments";
        return HMV_ERR_ARG;
    }
    if (hipSetDevice(device) != hipSuccess) { g_create_err = "hipSetDevice failed"; return HMV_ERR_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    HrFuseParams p{};
    p.N = N; p.H = H; p.W = W; p.C = C; p.ldc = C; p.nsrc = nsrc; p.relu = relu ? 1 : 0; p.f16 = f16 ? 1 : 0;
    std::vector<void *> owned, halves;   // halves: the fp16 copies the kernel reads, each framed by guard bands (op_guarded_alloc)
    auto release = [&]() {
        for (void *q : owned) (void)hipFree(q);
        for (void *q : halves) op_guarded_free(q);
    };
    auto fail = [&](int rc, const std::string &msg) {
        release();
        g_create_err = "hmv_op_hr_fuse_up: " + msg;
        return rc;
    };
    hipError_t e = hipSuccess;
    auto dev_copy = [&](const std::vector<float> &v) -> float * {
        void *d = nullptr;
        if (e == hipSuccess) e = hipMalloc(&d, v.size() * sizeof(float));
        if (e == hipSuccess) { owned.push_back(d); e = hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice); }
        return static_cast<float *>(d);
    };
    auto as_half = [&](const float *x, size_t rows, int ch) -> const void * {   // fp16 copy of fp32 rows
        void *d = nullptr;
        if (e == hipSuccess) e = op_guarded_alloc(&d, rows * ch * 2, s);
        if (e == hipSuccess) { halves.push_back(d); e = launch_rows_f32_to_half(x, d, rows, ch, 1, s); }
        return d;
    };
    for (int q = 0; q < nsrc; ++q) {
        HrFuseSrc &S = p.src[q];
        if (!src[q] || !w_host[q] || !bias_host[q] || src_c[q] <= 0 || shift[q] < 1 || shift[q] > 3) return fail(HMV_ERR_ARG, "bad source");
        S.C = src_c[q]; S.ld = src_c[q]; S.shift = shift[q]; S.H = H >> shift[q]; S.W = W >> shift[q];
        S.ldw = round_up(src_c[q], 32);
        std::vector<float> wp((size_t)round_up(C, 16) * S.ldw, 0.f), bp((size_t)round_up(C, 16), 0.f);   // rows / columns past C and C_s are zeros
        for (int o = 0; o < C; ++o) {
            for (int k = 0; k < S.C; ++k) wp[(size_t)o * S.ldw + k] = w_host[q][(size_t)o * S.C + k];
            bp[o] = bias_host[q][o];
        }
        S.w = dev_copy(wp);
        S.bias = dev_copy(bp);
        S.x = f16 ? as_half(src[q], (size_t)N * S.H * S.W, S.C) : static_cast<const void *>(src[q]);
    }
    p.base = f16 ? as_half(base, (size_t)N * H * W, C) : static_cast<const void *>(base);
    p.out = out;
    if (e != hipSuccess) return fail(HMV_ERR_HIP, hipGetErrorString(e));
    if (!hr_fuse_up_plan(p)) return fail(HMV_ERR_ARG, "the shape has no fused form (C % 4 (fp16: 8), C_s % 16, exact 2^shift map sizes, LDS)");
    e = launch_hr_fuse_up(p, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(HMV_ERR_HIP, hipGetErrorString(e));
    release();
    return HMV_OK;
}

// ------------------------------------------------------------------ the non-GEMM kernels of a forward, one launcher per entry
// (op-level float64 tests: tests/test_gpu_ops_f64.py).  Every operand is a device pointer of the caller; argument check, hipSetDevice, the
// launcher the engine itself calls, hipStreamSynchronize.  Nothing is allocated and nothing outlives the call.
namespace {
int op_bad(const char *who, const char *why) {
    g_create_err = std::string(who) + ": " + why;
    return HMV_ERR_ARG;
}
// Runs one launcher on `stream` of `device` and waits for it
template <class F>
int op_run(const char *who, int32_t device, void *stream, F &&launch) {
    if (hipSetDevice(device) != hipSuccess) { g_create_err = "hipSetDevice failed"; return HMV_ERR_HIP; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = launch(s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { g_create_err = std::string(who) + ": " + hipGetErrorString(e); return HMV_ERR_HIP; }
    return HMV_OK;
}
}  // namespace

extern "C" int hmv_op_input_layout(int32_t device, int32_t kind, int32_t mode, const float *x, int32_t N, int32_t H, int32_t W, void *out,
                                   int32_t *sat, void *stream) {
    static const char *who = "hmv_op_input_layout";
    if (!x || !out || N <= 0 || H <= 0 || W <= 0) return op_bad(who, "null operand or non-positive size");
    if (kind < 0 || kind > 1 || mode < 0 || mode > 2) return op_bad(who, "kind must be 0 (pixel rows) or 1 (space-to-depth), mode 0 (fp32), 1 (fp16) or 2 (split pairs)");
    return op_run(who, device, stream, [&](hipStream_t s) {
        if (kind == 1) return launch_nchw_to_s2d(x, out, N, H, W, mode, s, sat);
        if (mode == 2) return launch_nchw_to_nhwc_split(x, out, N, H, W, s, sat);
        if (mode == 1) return launch_nchw_to_nhwc8_f16(x, out, N, H, W, s);
        return launch_nchw_to_nhwc4(x, static_cast<float *>(out), N, H, W, s);
    });
}

extern "C" int hmv_op_maxpool(int32_t device, int32_t mode, const void *in, int32_t N, int32_t H, int32_t W, int32_t C, void *out, void *stream) {
    static const char *who = "hmv_op_maxpool";
    if (!in || !out || N <= 0 || H <= 0 || W <= 0 || C <= 0) return op_bad(who, "null operand or non-positive size");
    if (mode < 0 || mode > 2) return op_bad(who, "mode must be 0 (fp32), 1 (fp16) or 2 (split pairs)");
    if (C % (mode == 0 ? 4 : 8)) return op_bad(who, "C must be a multiple of 4 (fp32) or 8 (fp16, split pairs)");
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;   // MaxPool2d(3, 2, 1)
    return op_run(who, device, stream, [&](hipStream_t s) {
        if (mode == 2) return launch_maxpool3s2_split(in, out, N, H, W, C, Ho, Wo, s);
        if (mode == 1) return launch_maxpool3s2_f16(in, out, N, H, W, C, Ho, Wo, s);
        return launch_maxpool3s2(static_cast<const float *>(in), static_cast<float *>(out), N, H, W, C, Ho, Wo, s);
    });
}

extern "C" int hmv_op_soft_argmax(int32_t device, const float *hm, int32_t ld, int32_t N, int32_t h, int32_t w, float *coords, float *crop_img,
                                  float image_size, float heatmap_size, float *hm_nchw, void *stream) {
    static const char *who = "hmv_op_soft_argmax";
    if (!hm || !coords || !crop_img || N <= 0 || h <= 0 || w <= 0) return op_bad(who, "null operand or non-positive size");
    if (ld < 21 || (int64_t)N * 21 > INT32_MAX) return op_bad(who, "ld must hold the 21 joint channels");
    if (!(heatmap_size > 0.f)) return op_bad(who, "heatmap_size must be positive");
    return op_run(who, device, stream, [&](hipStream_t s) { return launch_soft_argmax(hm, ld, N, h, w, coords, crop_img, image_size, heatmap_size, hm_nchw, s); });
}

extern "C" int hmv_op_sample_gather(int32_t device, const void *feat, int32_t N, int32_t H, int32_t W, int32_t C, int32_t elem_bytes,
                                    const float *coords, void *out, void *stream) {
    static const char *who = "hmv_op_sample_gather";
    if (!feat || !coords || !out || N <= 0 || C <= 0) return op_bad(who, "null operand or non-positive size");
    if (H < 2 || W < 2) return op_bad(who, "maps of at least 2 x 2 pixels (grid_sample's own unnormalisation divides by size - 1)");
    if ((elem_bytes != 2 && elem_bytes != 4) || ((int64_t)C * elem_bytes) % 16) return op_bad(who, "elem_bytes 2 or 4, pixel rows of whole 16-byte chunks");
    return op_run(who, device, stream, [&](hipStream_t s) {
        return launch_sample_gather(static_cast<const float *>(feat), N, H, W, C, coords, static_cast<float *>(out), s, elem_bytes);
    });
}

extern "C" int hmv_op_sample_blend(int32_t device, const float *s4, int32_t lds4, int32_t C, int32_t N, int32_t H, int32_t W, const float *coords,
                                   float *tokens, int32_t ldt, int32_t col0, void *stream) {
    static const char *who = "hmv_op_sample_blend";
    if (!s4 || !coords || !tokens || N <= 0 || C <= 0) return op_bad(who, "null operand or non-positive size");
    if (H < 2 || W < 2) return op_bad(who, "maps of at least 2 x 2 pixels (grid_sample's own unnormalisation divides by size - 1)");
    if (lds4 < C || col0 < 0 || (int64_t)col0 + C > ldt) return op_bad(who, "lds4 >= C and columns [col0, col0 + C) inside a token row of ldt");
    return op_run(who, device, stream, [&](hipStream_t s) { return launch_sample_blend(s4, lds4, C, N, H, W, coords, tokens, ldt, col0, s); });
}

extern "C" int hmv_op_tokens_finalize(int32_t device, float *tokens, int32_t ldt, int32_t d, int32_t fdim, int32_t N, int32_t V, const int32_t *fpos,
                                      const float *coords, const float *bbox, const float *intr, int32_t pos_mask, const float *pe, float *raw_copy,
                                      void *pairs, int32_t *sat, void *stream) {
    static const char *who = "hmv_op_tokens_finalize";
    if (!tokens || N <= 0 || fdim <= 0) return op_bad(who, "null operand or non-positive size");
    if (pos_mask < 0 || pos_mask > 3) return op_bad(who, "pos_mask is 1 (pos2d) | 2 (crop FoV)");
    if (d != fdim + ((pos_mask & 1) ? 2 : 0) + ((pos_mask & 2) ? 10 : 0) || ldt < d) return op_bad(who, "d = fdim + 2 (pos2d) + 10 (crop FoV), d <= ldt");
    if (((pos_mask & 1) && !coords) || ((pos_mask & 2) && (!bbox || !intr))) return op_bad(who, "pos2d needs coords, the crop FoV needs bbox and intr");
    if (!fpos && V <= 0) return op_bad(who, "V must be positive in the uniform form");
    if (fpos && raw_copy) return op_bad(who, "the ragged form has no raw_copy");
    return op_run(who, device, stream, [&](hipStream_t s) {
        if (fpos) return launch_tokens_finalize_views(tokens, ldt, d, fdim, N, fpos, coords, bbox, intr, pos_mask, pe, s, pairs, sat);
        return launch_tokens_finalize(tokens, ldt, d, fdim, N, V, coords, bbox, intr, pos_mask, pe, raw_copy, s, pairs, sat);
    });
}

extern "C" int hmv_op_layernorm(int32_t device, const float *x, int32_t ldx, int32_t rows, int32_t d, const float *g1, const float *b1, float *y,
                                int32_t ldy, const float *g2, const float *b2, float *y2, void *stream) {
    static const char *who = "hmv_op_layernorm";
    if (!x || !g1 || !b1 || !y || rows <= 0 || d <= 0) return op_bad(who, "null operand or non-positive size");
    if (d > 1024 || ldy > 1024) return op_bad(who, "rows of at most 1024 columns (d, ldy)");
    if (ldx < d || ldy < d) return op_bad(who, "ldx >= d and ldy >= d");
    if ((g2 != nullptr) != (y2 != nullptr) || (b2 != nullptr) != (y2 != nullptr)) return op_bad(who, "the second norm takes g2, b2 and y2 together");
    return op_run(who, device, stream, [&](hipStream_t s) { return launch_layernorm(x, ldx, rows, d, g1, b1, y, ldy, g2, b2, y2, s); });
}

namespace {
const char *splitk_args_bad(const float *slab, int32_t S, int32_t rows, int32_t lds, int32_t N, const float *bias, const float *res, int32_t ldr,
                            int32_t rg_out, int32_t rg_in, const void *out, int32_t ldc) {
    if (!slab || !bias || !out || rows <= 0 || N <= 0) return "null operand or non-positive size";
    if (S < 1) return "S must be positive";
    if (lds < N || ldc < N || (res && ldr < N)) return "lds, ldc and ldr must hold N columns";
    if (rg_out < 0 || (rg_out > 0 && rg_in < rg_out)) return "residual row groups: rg_out = 0, or 0 < rg_out <= rg_in";
    return nullptr;
}
}  // namespace

extern "C" int hmv_op_splitk_reduce(int32_t device, const float *slab, int32_t S, int32_t rows, int32_t lds, int32_t N, const float *bias,
                                    const float *res, int32_t ldr, int32_t rg_out, int32_t rg_in, int32_t act, float *out, int32_t ldc, void *stream) {
    static const char *who = "hmv_op_splitk_reduce";
    if (const char *why = splitk_args_bad(slab, S, rows, lds, N, bias, res, ldr, rg_out, rg_in, out, ldc)) return op_bad(who, why);
    if (act < ACT_NONE || act > ACT_LEAKY) return op_bad(who, "act must be 0 (none), 1 (ReLU), 2 (GELU) or 3 (LeakyReLU)");
    return op_run(who, device, stream, [&](hipStream_t s) { return launch_splitk_reduce(slab, S, rows, lds, N, bias, res, ldr, rg_out, rg_in, act, out, ldc, s); });
}

extern "C" int hmv_op_splitk_layernorm(int32_t device, const float *slab, int32_t S, int32_t rows, int32_t lds, int32_t d, const float *bias,
                                       const float *res, int32_t ldr, int32_t rg_out, int32_t rg_in, const float *g1, const float *b1, float *y,
                                       int32_t ldy, const float *g2, const float *b2, float *y2, void *stream) {
    static const char *who = "hmv_op_splitk_layernorm";
    if (const char *why = splitk_args_bad(slab, S, rows, lds, d, bias, res, ldr, rg_out, rg_in, y, ldy)) return op_bad(who, why);
    if (S != 4) return op_bad(who, "the fused form exists for S = 4 slices only");
    if (!g1 || !b1) return op_bad(who, "null operand or non-positive size");
    if (d > 1024 || ldy > 1024) return op_bad(who, "rows of at most 1024 columns (d, ldy)");
    if ((g2 != nullptr) != (y2 != nullptr) || (b2 != nullptr) != (y2 != nullptr)) return op_bad(who, "the second norm takes g2, b2 and y2 together");
    return op_run(who, device, stream, [&](hipStream_t s) {
        return launch_splitk_layernorm(slab, S, rows, lds, d, bias, res, ldr, rg_out, rg_in, g1, b1, y, ldy, g2, b2, y2, s);
    });
}

extern "C" int hmv_op_add_pe(int32_t device, const float *x, int32_t ldx, int32_t rows, int32_t T, const int32_t *fpos, int32_t d, const float *pe,
                             float *y, int32_t ldy, void *stream) {
    static const char *who = "hmv_op_add_pe";
    if (!x || !pe || !y || rows <= 0 || d <= 0) return op_bad(who, "null operand or non-positive size");
    if (ldx < d || ldy < d) return op_bad(who, "ldx >= d and ldy >= d");
    if (!fpos && T <= 0) return op_bad(who, "T must be positive in the uniform form");
    if (fpos && rows % 21) return op_bad(who, "the ragged form takes whole frames: rows % 21 == 0");
    return op_run(who, device, stream, [&](hipStream_t s) {
        if (fpos) return launch_add_pe_views(x, ldx, rows, fpos, d, pe, y, ldy, s);
        return launch_add_pe(x, ldx, rows, T, d, pe, y, ldy, s);
    });
}

extern "C" int hmv_op_cheb_mix(int32_t device, const float *y, int32_t ldy, int32_t B, int32_t co, const float *tk, const float *bias, int32_t leaky,
                               float *out, int32_t ldo, void *stream) {
    static const char *who = "hmv_op_cheb_mix";
    if (!y || !tk || !bias || !out || B <= 0 || co <= 0) return op_bad(who, "null operand or non-positive size");
    if ((int64_t)3 * co > ldy || ldo < co) return op_bad(who, "ldy >= 3 co and ldo >= co");
    if ((co + 31) / 32 > 65535) return op_bad(who, "co beyond the launch grid");
    return op_run(who, device, stream, [&](hipStream_t s) { return launch_cheb_mix(y, ldy, B, co, tk, bias, leaky, out, ldo, s); });
}

// ------------------------------------------------------------------ the fused tail kernels (fusion_kernels.hip), each behind the launcher the
// engine calls (op-level float64 tests: tests/test_gpu_tail_f64.py)
extern "C" int hmv_op_ff_block(int32_t device, hmv_ff_block_args *a, void *stream) {
    static const char *who = "hmv_op_ff_block";
    if (!a) return op_bad(who, "args is NULL");
    if (a->struct_size != (int32_t)sizeof(hmv_ff_block_args)) return op_bad(who, "struct_size does not match this library's hmv_ff_block_args");
    if (a->rows <= 0 || a->d <= 0) return op_bad(who, "null operand or non-positive size");
    if (!a->out || !a->w1 || !a->w2 || !a->b1 || !a->b2 || !a->fg || !a->fb) return op_bad(who, "out, w1, w2, b1, b2, fg and fb must not be NULL");
    if ((a->n1g != nullptr) != (a->n1b != nullptr) || (a->n2g != nullptr) != (a->n2b != nullptr)) return op_bad(who, "a norm takes its gamma and beta together");
    if ((a->slab != nullptr) == (a->x != nullptr)) return op_bad(who, "exactly one source: slab or x");
    if (a->tile_rows != 0 && a->tile_rows != 16 && a->tile_rows != 32) return op_bad(who, "tile_rows must be 0 (the launcher's rule), 16 or 32");
    FfBlockParams p{};
    p.slab = a->slab; p.S = a->S; p.slice = a->slice > 0 ? (size_t)a->slice : 0; p.lds = a->lds; p.bias0 = a->bias0;
    p.res = a->slab ? a->res : nullptr; p.ldr = a->ldr; p.rg_out = a->rg_out; p.rg_in = a->rg_in;
    p.x = a->x; p.ldx = a->ldx;
    p.rows = a->rows; p.d = a->d; p.ld = a->ld;
    p.n1g = a->n1g; p.n1b = a->n1b; p.fg = a->fg; p.fb = a->fb; p.n2g = a->n2g; p.n2b = a->n2b;
    p.w1 = a->w1; p.b1 = a->b1; p.ldw1 = a->ldw1; p.w2 = a->w2; p.b2 = a->b2; p.ldw2 = a->ldw2;
    p.out = a->out; p.ldo = a->ldo; p.hid = a->hid; p.out_pairs = a->out_pairs; p.sat = a->sat;
    if (const char *why = ff_block_refusal(p)) return op_bad(who, why);
    if (a->slab && (a->lds < a->d || (a->S > 1 && a->slice < (int64_t)a->rows * a->lds))) return op_bad(who, "lds >= d, and slices of at least rows * lds floats");
    if (p.res && (a->ldr < a->d || a->rg_out < 0 || (a->rg_out > 0 && a->rg_in < a->rg_out)))
        return op_bad(who, "ldr >= d; residual row groups: rg_out = 0, or 0 < rg_out <= rg_in");
    if (a->x && a->ldx < a->d) return op_bad(who, "ldx >= d");
    if (a->tile_rows == 32 && ff_block_lds_bytes(p, 32) > (size_t)160 * 1024) return op_bad(who, "a 32-row tile of this ld and hid does not fit 160 KB of LDS");
    int used = 0;
    const int rc = op_run(who, device, stream, [&](hipStream_t s) { return launch_ff_block(p, s, a->tile_rows, &used); });
    if (rc == HMV_OK) a->tile_rows_used = used;
    return rc;
}

extern "C" int hmv_op_cheb_fused(int32_t device, const hmv_cheb_fused_args *a, void *stream) {
    static const char *who = "hmv_op_cheb_fused";
    if (!a) return op_bad(who, "args is NULL");
    if (a->struct_size != (int32_t)sizeof(hmv_cheb_fused_args)) return op_bad(who, "struct_size does not match this library's hmv_cheb_fused_args");
    if (!a->x || !a->w1 || !a->bias1 || !a->w2 || !a->bias2 || !a->w3 || !a->bias3 || !a->tk || !a->scratch || !a->out)
        return op_bad(who, "null operand or non-positive size");
    if (a->B <= 0 || a->K <= 0 || a->c1 <= 0 || a->c2 <= 0 || a->c3 <= 0 || (int64_t)a->B * 21 > INT32_MAX) return op_bad(who, "null operand or non-positive size");
    if (!cheb_fusable(a->K, a->ldx, a->ldw1, a->c1, a->ldw2, a->c2, a->ldw3, a->c3))
        return op_bad(who, "the shape has no fused form (K <= 576, c1 <= 256, c2 <= 64, each a multiple of 16; c3 <= 5; ldx, ldw1 >= K, ldw2 >= c1, ldw3 >= c2, multiples of 4)");
    if (a->ldo < a->c3) return op_bad(who, "ldo >= c3");
    ChebFusedParams p{};
    p.x = a->x; p.ldx = a->ldx; p.B = a->B; p.K = a->K;
    p.w1 = a->w1; p.ldw1 = a->ldw1; p.c1 = a->c1; p.bias1 = a->bias1;
    p.w2 = a->w2; p.ldw2 = a->ldw2; p.c2 = a->c2; p.bias2 = a->bias2;
    p.w3 = a->w3; p.ldw3 = a->ldw3; p.c3 = a->c3; p.bias3 = a->bias3;
    p.tk = a->tk; p.scratch = a->scratch; p.out = a->out; p.ldo = a->ldo;
    return op_run(who, device, stream, [&](hipStream_t s) { return launch_cheb_fused(p, s); });
}
