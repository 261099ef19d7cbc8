// Body of attention_mfma_kernel<D, ATT_WAVES> and attention_mfma_views_kernel<D, ATT_WAVES> (misc_kernels.hip), included once by each.
// The includer defines ATT_ROWS -- statements that leave qb / kb / vb (the sample's first query / key / value row at head h) and, where they
// are not kernel arguments, Tq / Tk in scope -- and ATT_OROW, the output row of query `row`.  The chunk split (by Tk alone), the
// recurrence and the merge are the same text for both.  Textual sharing rather than a device function, so that the uniform kernel's
// code is the compiler's output for exactly the token sequence it always had.
    using SH = AttShape<D, ATT_WAVES>;
    constexpr int NC = SH::NC, NU = D / 8, NV = D / 32;   // K vectors per lane, V vectors per lane and quarter chunk
    extern __shared__ __attribute__((aligned(16))) float att_smem[];
    const int qblk = blockIdx.x % nqb, bh = blockIdx.x / nqb;
    const int b = bh >> 3, h = bh & 7;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, kh = lane >> 5;
    const size_t ld = (size_t)kv_ld;
    ATT_ROWS
    const int nkc = (Tk + 31) >> 5;
    const float scale = D == 128 ? 0.08838834764831845f : 0.0625f;  // D ** -0.5
    float *sQ = att_smem;                                                   // [32][LDK]
    float *sVw = att_smem + SH::Q_FLOATS + wave * SH::V_FLOATS;             // [8][D], this wave's

    // every global load of a wave's first chunk is issued before anything waits
    constexpr bool PREFETCH = D == 128;
    f32x4 kf[NU], va[NV], vb_[NV];
    int kc = wave;
#define ATT_LOAD_K(KC)                                                                                  \
    do {                                                                                                \
        const int key_ = (KC) * 32 + l31;                                                               \
        const bool kv_ = key_ < Tk;                                                                     \
        const float *krow_ = kb + (size_t)(kv_ ? key_ : 0) * ld + 4 * kh;                               \
        _Pragma("unroll") for (int u = 0; u < NU; ++u) {                                                \
            kf[u] = *reinterpret_cast<const f32x4 *>(krow_ + 8 * u);                                    \
            if (!kv_) kf[u] = f32x4{0.f, 0.f, 0.f, 0.f};                                                \
        }                                                                                               \
    } while (0)
    // 8 keys x D channels: NV coalesced 16-byte vectors per lane (keys >= Tk are zeros)
#define ATT_LOAD_V(KEY0, VR)                                                                            \
    do {                                                                                                \
        _Pragma("unroll") for (int it = 0; it < NV; ++it) {                                             \
            const int idx_ = it * 64 + lane, k2_ = (KEY0) + idx_ / (D / 4);                             \
            VR[it] = f32x4{0.f, 0.f, 0.f, 0.f};                                                         \
            if (k2_ < Tk) VR[it] = *reinterpret_cast<const f32x4 *>(vb + (size_t)k2_ * ld + 4 * (idx_ % (D / 4))); \
        }                                                                                               \
    } while (0)
#define ATT_STORE_V(VR)                                                                                 \
    do {                                                                                                \
        __builtin_amdgcn_wave_barrier();                                                                \
        _Pragma("unroll") for (int it = 0; it < NV; ++it) {                                             \
            const int idx_ = it * 64 + lane;                                                            \
            *reinterpret_cast<f32x4 *>(&sVw[(idx_ / (D / 4)) * D + 4 * (idx_ % (D / 4))]) = VR[it];     \
        }                                                                                               \
        __builtin_amdgcn_wave_barrier();                                                                \
    } while (0)
    // O^T += V^T P^T over the 8 keys of quarter G: the k-pair of step e2 is (key 8G + e2, key 8G + e2 + 4) = P register 4G + e2
#define ATT_PV(G)                                                                                       \
    do {                                                                                                \
        _Pragma("unroll") for (int e2 = 0; e2 < 4; ++e2) {                                              \
            const float *vrow = &sVw[(4 * kh + e2) * D + l31];                                          \
            _Pragma("unroll") for (int c = 0; c < NC; ++c)                                              \
                o[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(vrow[32 * c], sacc[4 * (G) + e2], o[c], 0, 0, 0); \
        }                                                                                               \
    } while (0)
    if (kc < nkc) {
        ATT_LOAD_K(kc);
        ATT_LOAD_V(kc * 32, va);
    }
    // Q block (rows >= Tq are zeros), shared by the waves
#pragma unroll
    for (int it = 0; it < (8 * D) / (64 * ATT_WAVES); ++it) {
        const int idx = it * (64 * ATT_WAVES) + tid, r = idx / (D / 4), c4 = idx % (D / 4), row = qblk * 32 + r;
        f32x4 qv = {0.f, 0.f, 0.f, 0.f};
        if (row < Tq) qv = *reinterpret_cast<const f32x4 *>(qb + (size_t)row * q_ld + 4 * c4);
        *reinterpret_cast<f32x4 *>(&sQ[r * SH::LDK + 4 * c4]) = qv;
    }
    __syncthreads();

    f32x16 o[NC];   // o[c][e] on lane (q, half): O[q][32c + (e&3) + 8(e>>2) + 4 half]
    float m_run = -INFINITY, l_run = 0.f;   // of query l31, over the keys this lane has seen (its half of every chunk)
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[c][e] = 0.f;

#define ATT_CHUNK(KC)                                                                                   \
    do {                                                                                                \
        f32x16 sacc;                                                                                    \
        _Pragma("unroll") for (int e = 0; e < 16; ++e) sacc[e] = 0.f;                                   \
        _Pragma("unroll") for (int u = 0; u < NU; ++u) {                                                \
            const f32x4 qf = *reinterpret_cast<const f32x4 *>(&sQ[l31 * SH::LDK + 8 * u + 4 * kh]);     \
            _Pragma("unroll") for (int e = 0; e < 4; ++e)                                               \
                sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[u][e], qf[e], sacc, 0, 0, 0);            \
        }                                                                                               \
        /* the key rows of this wave's NEXT chunk fly during the softmax and the P V products of this one (their registers are free) */ \
        if (PREFETCH && (KC) + ATT_WAVES < nkc) ATT_LOAD_K((KC) + ATT_WAVES);                           \
        ATT_LOAD_V((KC) * 32 + 8, vb_);   /* the next 8 keys fly during the softmax */                  \
        /* register e = key (e&3) + 8(e>>2) + 4 half of the chunk, for query l31 */                     \
        float mx = -INFINITY;                                                                           \
        _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                \
            const bool kv_ = (KC) * 32 + (e & 3) + 8 * (e >> 2) + 4 * kh < Tk;                          \
            sacc[e] = kv_ ? sacc[e] * scale : -INFINITY;                                                \
            mx = fmaxf(mx, sacc[e]);                                                                    \
        }                                                                                               \
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));          /* finite: the chunk has >= 1 valid key */     \
        const float m_new = fmaxf(m_run, mx);                                                           \
        const float alpha = expf(m_run - m_new);         /* exp(-inf) = 0 on the first chunk */         \
        float psum = 0.f;                                                                               \
        _Pragma("unroll") for (int e = 0; e < 16; ++e) {                                                \
            sacc[e] = expf(sacc[e] - m_new);             /* exp(-inf) = 0 for keys >= Tk */             \
            psum += sacc[e];                                                                            \
        }                                                                                               \
        l_run = l_run * alpha + psum;                                                                   \
        m_run = m_new;                                                                                  \
        _Pragma("unroll") for (int c = 0; c < NC; ++c)                                                  \
            _Pragma("unroll") for (int e = 0; e < 16; ++e) o[c][e] *= alpha;                            \
        /* 8 keys at a time through the wave's LDS buffer; the loads run two quarters ahead */          \
        ATT_STORE_V(va);                                                                                \
        ATT_LOAD_V((KC) * 32 + 16, va);                                                                 \
        ATT_PV(0);                                                                                      \
        ATT_STORE_V(vb_);                                                                               \
        ATT_LOAD_V((KC) * 32 + 24, vb_);                                                                \
        ATT_PV(1);                                                                                      \
        ATT_STORE_V(va);                                                                                \
        if (PREFETCH && (KC) + ATT_WAVES < nkc) ATT_LOAD_V(((KC) + ATT_WAVES) * 32, va);   /* ... and its first 8 value rows */ \
        ATT_PV(2);                                                                                      \
        ATT_STORE_V(vb_);                                                                               \
        ATT_PV(3);                                                                                      \
        __builtin_amdgcn_wave_barrier();                                                                \
    } while (0)
    if (kc < nkc) {
        // 128-wide heads: a chunk requests the operands of this wave's next one (round 4); the 256-wide ones have no registers for that
        if constexpr (PREFETCH) {
            for (; kc < nkc; kc += ATT_WAVES) ATT_CHUNK(kc);
        } else {
            ATT_CHUNK(kc);
            for (kc += ATT_WAVES; kc < nkc; kc += ATT_WAVES) {
                ATT_LOAD_K(kc);
                ATT_LOAD_V(kc * 32, va);
                ATT_CHUNK(kc);
            }
        }
    }
#undef ATT_CHUNK
#undef ATT_LOAD_K
#undef ATT_LOAD_V
#undef ATT_STORE_V
#undef ATT_PV

    // ---- merge the 4 waves' partials in wave order: out = sum_w O_w e^(m_w - M) / sum_w l_w e^(m_w - M)
    __syncthreads();   // the merge area aliases the loop's buffers
    float *sO = att_smem, *sM = att_smem + ATT_WAVES * NC * 16 * 64, *sL = sM + ATT_WAVES * 32;
    l_run += __shfl_xor(l_run, 32, 64);
    if (kh == 0) { sM[wave * 32 + l31] = m_run; sL[wave * 32 + l31] = l_run; }
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) sO[((wave * NC + c) * 16 + e) * 64 + lane] = o[c][e];
    __syncthreads();
    {
        float M = sM[l31];
#pragma unroll
        for (int w = 1; w < ATT_WAVES; ++w) M = fmaxf(M, sM[w * 32 + l31]);
        float a[ATT_WAVES], den = 0.f;
#pragma unroll
        for (int w = 0; w < ATT_WAVES; ++w) {
            a[w] = expf(sM[w * 32 + l31] - M);   // exp(-inf) = 0 for a wave that had no chunk
            den += sL[w * 32 + l31] * a[w];
        }
        const float inv = 1.f / den;
        const int row = qblk * 32 + l31;
#pragma unroll
        for (int c = wave; c < NC; c += ATT_WAVES) {   // this wave finishes channel blocks wave, wave + 4, ..
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 r4;
#pragma unroll
                for (int e2 = 0; e2 < 4; ++e2) {
                    float num = 0.f;
#pragma unroll
                    for (int w = 0; w < ATT_WAVES; ++w) num += sO[((w * NC + c) * 16 + 4 * g + e2) * 64 + lane] * a[w];
                    r4[e2] = num * inv;
                }
                if (row < Tq) {
                    if (pairs) {   // the rows as (hi, lo) fp16 pairs [hi 8 D | lo 8 D] for a split-pair to_out GEMM (gemm_x3.hip): split_f16's arithmetic
                        f16x4 hi4, lo4;
                        bool ov = false;
#pragma unroll
                        for (int e2 = 0; e2 < 4; ++e2) {
                            _Float16 a_, b_;
                            ov |= split_f16(r4[e2], a_, b_);
                            hi4[e2] = a_; lo4[e2] = b_;
                        }
                        note_range(sat, ov);
                        _Float16 *pr = reinterpret_cast<_Float16 *>(out) + (ATT_OROW) * (16 * D) + h * D + 32 * c + 8 * g + 4 * kh;
                        *reinterpret_cast<f16x4 *>(pr) = hi4;
                        *reinterpret_cast<f16x4 *>(pr + 8 * D) = lo4;
                    } else {
                        *reinterpret_cast<f32x4 *>(out + (ATT_OROW) * (8 * D) + h * D + 32 * c + 8 * g + 4 * kh) = r4;
                    }
                }
            }
        }
    }
