// Attention maps of the fusion blocks (the reference's return_attention=True, layers.py:202-237 / 267-301): the softmax the forward's
// flash-style kernels (misc_kernels.hip) never write.  Launched only behind hmv_set_attention_capture; the forward's kernels are untouched.
//
// attention_probs_kernel<D, PAIRS>: one workgroup (4 waves) per (sample, head, 32-query block), as in attention_mfma_kernel.  The 32-key
// chunks of the sample's key range are dealt round-robin to the waves, by the sample's own Tk alone, so a sample's bits never depend on
// its batch.  Logits as the forward computes them: S^T = K_chunk Q_blk^T on v_mfma_f32_32x32x2f32, A = the lane's own key row from global
// memory, B = the Q block from LDS, the k order of ATT_CHUNK, the same D ** -0.5, keys >= Tk at -inf.  Two passes over the keys, so that
// no buffer grows with Tk:
//   pass 1  running row maximum and sum per wave (the forward's recurrence without the P V product), merged across the waves in wave
//           order through LDS: M = max_w m_w, den = sum_w l_w e^(m_w - M)
//   pass 2  the same logits again (the same device function: one dependent MFMA chain per chunk, hence the same bits), then
//           p = e^(s - M) * (1 / den).  The 32 x 32 tile is transposed through a per-wave LDS buffer, so that a half wave stores 32
//           consecutive keys of one row; rows hold 21 n floats, so every store is a single 4-byte one.
// PAIRS (D = 128): q and k rows are the (hi, lo) fp16 pairs [hi | lo] that the projection GEMMs of the fp16-kernel modes leave behind;
// the loaders form float(hi) + float(lo) -- exact in fp32 -- and everything behind them is the fp32 arithmetic above.  The maps of those
// modes are therefore fp32 arithmetic on the forward's own operands, not the registers of attention_x3_kernel.
//
// attention_share_kernel: share[b][h][i][r] = sum of the 21 probabilities that query i spends on the view of rank r, in key order, read
// back from the map (one thread per output, no atomics).
#include "kernels.h"

namespace hmv {

typedef float pf32x4 __attribute__((ext_vector_type(4)));
typedef float pf32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 pf16x4 __attribute__((ext_vector_type(4)));

namespace {

// The rows of sample b and the extents of its map (AttnProbsRows, kernels.h).  false: nothing to do for this (b, qblk) -- the query block
// lies beyond the sample's queries, or the sample has no keys (one view in the cross block: its rows of the map stay the zeros the call
// filled in).  The answer depends on (b, qblk) alone, so a whole workgroup takes it, ahead of any LDS access or barrier.
__device__ __forceinline__ bool probs_rows(const AttnProbsRows &pr, int b, int qblk, size_t &q0, size_t &k0, int &Tq, int &Tk) {
    if (pr.seg) {
        const int r0 = pr.seg[b], Tb = pr.seg[b + 1] - r0;
        Tq = pr.tq_fixed ? pr.tq_fixed : Tb;
        Tk = Tb - pr.koff;
        q0 = pr.q_seg ? (size_t)r0 : 0;
        k0 = (size_t)(r0 + pr.koff);
    } else {
        Tq = pr.Tq;
        Tk = pr.Tk;
        q0 = (size_t)b * pr.q_bstride;
        k0 = (size_t)b * pr.T + pr.koff;
    }
    return qblk * 32 < Tq && Tk > 0;
}

// four consecutive channels of a row: fp32, or float(hi) + float(lo) of a pair row (lo_off halfs behind the hi plane)
template <bool PAIRS>
__device__ __forceinline__ pf32x4 probs_load4(const void *row, int c, int lo_off) {
    if constexpr (PAIRS) {
        const _Float16 *p = static_cast<const _Float16 *>(row) + c;
        const pf16x4 hi = *reinterpret_cast<const pf16x4 *>(p), lo = *reinterpret_cast<const pf16x4 *>(p + lo_off);
        return pf32x4{(float)hi[0] + (float)lo[0], (float)hi[1] + (float)lo[1], (float)hi[2] + (float)lo[2], (float)hi[3] + (float)lo[3]};
    } else {
        return *reinterpret_cast<const pf32x4 *>(static_cast<const float *>(row) + c);
    }
}

// The scaled, masked logits of chunk kc for query l31 against 16 of its 32 keys: register e = key (e & 3) + 8 (e >> 2) + 4 kh of the chunk.
// Both passes call this; the accumulator is one dependent chain, so its bits do not depend on how the loads around it are scheduled.
template <int D, bool PAIRS>
__device__ __forceinline__ pf32x16 probs_logits(const char *kb, size_t k_row_bytes, int lo_off, const float *sQ, int kc, int Tk, int l31, int kh) {
    constexpr int LDK = D + 4, NU = D / 8;
    const float scale = D == 128 ? 0.08838834764831845f : 0.0625f;   // D ** -0.5
    const int key = kc * 32 + l31;
    const bool kv = key < Tk;
    const void *krow = kb + (size_t)(kv ? key : 0) * k_row_bytes;
    pf32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        pf32x4 kf = probs_load4<PAIRS>(krow, 8 * u + 4 * kh, lo_off);
        if (!kv) kf = pf32x4{0.f, 0.f, 0.f, 0.f};
        const pf32x4 qf = *reinterpret_cast<const pf32x4 *>(&sQ[l31 * LDK + 8 * u + 4 * kh]);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[e], qf[e], acc, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const bool v = kc * 32 + (e & 3) + 8 * (e >> 2) + 4 * kh < Tk;
        acc[e] = v ? acc[e] * scale : -INFINITY;
    }
    return acc;
}

constexpr int PROBS_WAVES = 4, PROBS_TLD = 33;   // tile row stride: the transposing writes of a half wave fall on 32 banks

// q / k: first row at head 0 (fp32, or the hi plane of pair rows); q_ld / kv_ld / lo_off in elements of that type.
// probs [B][8][pr.Tq_pad][pr.Tk_pad]
template <int D, bool PAIRS>
__global__ __launch_bounds__(64 * PROBS_WAVES) void attention_probs_kernel(const void *__restrict__ q, int q_ld, const void *__restrict__ k, int kv_ld,
                                                                           int lo_off, const AttnProbsRows pr, int nqb, float *__restrict__ probs) {
    constexpr int LDK = D + 4;
    constexpr size_t ES = PAIRS ? 2 : 4;
    const int qblk = blockIdx.x % nqb, bh = blockIdx.x / nqb;
    const int b = bh >> 3, h = bh & 7;
    size_t q0, k0;
    int Tq, Tk;
    if (!probs_rows(pr, b, qblk, q0, k0, Tq, Tk)) return;
    __shared__ __attribute__((aligned(16))) float sQ[32 * LDK];
    __shared__ float sM[PROBS_WAVES * 32], sL[PROBS_WAVES * 32];
    __shared__ float sT[PROBS_WAVES * 32 * PROBS_TLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, kh = lane >> 5;
    const char *qb = static_cast<const char *>(q) + (q0 * q_ld + (size_t)h * D) * ES;
    const char *kb = static_cast<const char *>(k) + (k0 * kv_ld + (size_t)h * D) * ES;
    const size_t k_row_bytes = (size_t)kv_ld * ES;
    const int nkc = (Tk + 31) >> 5;

    // Q block (rows >= Tq are zeros), shared by the waves
#pragma unroll
    for (int it = 0; it < (8 * D) / (64 * PROBS_WAVES); ++it) {
        const int idx = it * (64 * PROBS_WAVES) + tid, r = idx / (D / 4), c4 = idx % (D / 4), row = qblk * 32 + r;
        pf32x4 qv = {0.f, 0.f, 0.f, 0.f};
        if (row < Tq) qv = probs_load4<PAIRS>(qb + (size_t)row * q_ld * ES, 4 * c4, lo_off);
        *reinterpret_cast<pf32x4 *>(&sQ[r * LDK + 4 * c4]) = qv;
    }
    __syncthreads();

    // ---- pass 1: this wave's running maximum and sum of query l31 (the lane's half of every chunk; the halves meet below)
    float m_run = -INFINITY, l_run = 0.f;
    for (int kc = wave; kc < nkc; kc += PROBS_WAVES) {
        const pf32x16 s = probs_logits<D, PAIRS>(kb, k_row_bytes, lo_off, sQ, kc, Tk, l31, kh);
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s[e]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));   // finite: the chunk has >= 1 valid key
        const float m_new = fmaxf(m_run, mx);
        const float alpha = expf(m_run - m_new);   // exp(-inf) = 0 on the first chunk
        float psum = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) psum += expf(s[e] - m_new);   // exp(-inf) = 0 for keys >= Tk
        l_run = l_run * alpha + psum;
        m_run = m_new;
    }
    l_run += __shfl_xor(l_run, 32, 64);
    if (kh == 0) { sM[wave * 32 + l31] = m_run; sL[wave * 32 + l31] = l_run; }
    __syncthreads();
    float M = sM[l31];
#pragma unroll
    for (int w = 1; w < PROBS_WAVES; ++w) M = fmaxf(M, sM[w * 32 + l31]);
    float den = 0.f;
#pragma unroll
    for (int w = 0; w < PROBS_WAVES; ++w) den += sL[w * 32 + l31] * expf(sM[w * 32 + l31] - M);   // exp(-inf) = 0 for a wave that had no chunk
    const float inv = 1.f / den;

    // ---- pass 2: the probabilities of this wave's chunks, transposed through the wave's tile and stored row by row
    float *tile = sT + wave * 32 * PROBS_TLD;
    float *orow0 = probs + ((size_t)bh * pr.Tq_pad + (size_t)qblk * 32) * pr.Tk_pad;
    const int Tq_st = Tq < pr.Tq_pad ? Tq : pr.Tq_pad, Tk_st = Tk < pr.Tk_pad ? Tk : pr.Tk_pad;   // (the map's extents bound every store)
    for (int kc = wave; kc < nkc; kc += PROBS_WAVES) {
        const pf32x16 s = probs_logits<D, PAIRS>(kb, k_row_bytes, lo_off, sQ, kc, Tk, l31, kh);
#pragma unroll
        for (int e = 0; e < 16; ++e) tile[l31 * PROBS_TLD + (e & 3) + 8 * (e >> 2) + 4 * kh] = expf(s[e] - M) * inv;
        __builtin_amdgcn_wave_barrier();
        const int key = kc * 32 + l31;
#pragma unroll
        for (int it = 0; it < 16; ++it) {
            const int r = 2 * it + kh;
            const float p = tile[r * PROBS_TLD + l31];
            if (qblk * 32 + r < Tq_st && key < Tk_st) orow0[(size_t)r * pr.Tk_pad + key] = p;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// one thread per share[b][h][i][r]; rank0: the view rank of key 0 (1 in cross_attn's cross block, whose rank-0 view supplies the queries)
__global__ void attention_share_kernel(const float *__restrict__ probs, const AttnProbsRows pr, int rank0, int views, size_t total, float *__restrict__ share) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int r = (int)(idx % views), i = (int)((idx / views) % pr.Tq_pad);
    const size_t bh = idx / ((size_t)views * pr.Tq_pad);
    size_t q0, k0;
    int Tq, Tk;
    (void)probs_rows(pr, (int)(bh >> 3), 0, q0, k0, Tq, Tk);
    float s = 0.f;
    const int j0 = (r - rank0) * 21;
    if (i < Tq && r >= rank0 && j0 + 21 <= Tk) {
        const float *row = probs + (bh * pr.Tq_pad + i) * pr.Tk_pad + j0;
        for (int j = 0; j < 21; ++j) s += row[j];
    }
    share[idx] = s;
}

template <int D, bool PAIRS>
hipError_t launch_probs(const void *q, int q_ld, const void *k, int kv_ld, int lo_off, int B, const AttnProbsRows &pr, float *probs, hipStream_t s) {
    const int nqb = (pr.Tq_pad + 31) >> 5;
    hipLaunchKernelGGL((attention_probs_kernel<D, PAIRS>), dim3((unsigned)B * 8 * nqb), dim3(64 * PROBS_WAVES), 0, s, q, q_ld, k, kv_ld, lo_off, pr, nqb, probs);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_attention_probs(int kind, const void *q, int q_ld, const void *k, int kv_ld, int B, const AttnProbsRows &pr, float *probs, hipStream_t s) {
    if (!q || !k || !probs || B <= 0 || pr.Tq_pad <= 0 || pr.Tk_pad <= 0 || kind < 0 || kind > 2) return hipErrorInvalidValue;
    if (!pr.seg && (pr.Tq <= 0 || pr.Tk <= 0 || pr.Tq > pr.Tq_pad || pr.Tk > pr.Tk_pad)) return hipErrorInvalidValue;
    if (kind == 0) return launch_probs<128, false>(q, q_ld, k, kv_ld, 0, B, pr, probs, s);
    if (kind == 1) return launch_probs<128, true>(q, q_ld, k, kv_ld, q_ld / 2, B, pr, probs, s);   // rows [hi | lo]: the lo plane half a row on
    return launch_probs<256, false>(q, q_ld, k, kv_ld, 0, B, pr, probs, s);
}

hipError_t launch_attention_share(const float *probs, int B, const AttnProbsRows &pr, int rank0, int views, float *share, hipStream_t s) {
    if (!probs || !share || B <= 0 || views <= 0 || rank0 < 0 || pr.Tq_pad <= 0 || pr.Tk_pad <= 0) return hipErrorInvalidValue;
    const size_t total = (size_t)B * 8 * pr.Tq_pad * views;
    hipLaunchKernelGGL(attention_share_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, probs, pr, rank0, views, total, share);
    return hipGetLastError();
}

}  // namespace hmv
