// Body of attention_x3_kernel and attention_x3_views_kernel (misc_kernels.hip), included once by each: AX_ROWS / AX_OROW as ATT_ROWS /
// ATT_OROW of attention_mfma_body.inc.
    constexpr int D = 128, NC = 4;
    extern __shared__ __attribute__((aligned(16))) char ax_smem[];
    const int qblk = blockIdx.x % nqb, bh = blockIdx.x / nqb;
    const int b = bh >> 3, h = bh & 7;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, kh = lane >> 5;
    const size_t ld = (size_t)kv_ld;
    AX_ROWS
    const int nkc = (Tk + 31) >> 5;
    const float scale = 0.08838834764831845f;   // 128 ** -0.5
    _Float16 *sQ = reinterpret_cast<_Float16 *>(ax_smem);                                   // [2][32][AX_QLD]
    _Float16 *sVw = sQ + AX_Q_HALFS + wave * AX_V_HALFS;                                    // [2][16][AX_VLD], this wave's

    f16x8 kh8[8], kl8[8], vh8[4], vl8[4];   // the chunk's key rows (8 steps x (hi, lo)); 16 of its value rows (16 keys x 128 channels = 4 + 4 vectors per lane)
    int kc = wave;
    // (keys >= Tk read the last valid row: their logits are set to -inf and their P to exactly 0 below, so only finiteness matters)
#define AX_LOAD_K(KC)                                                                                   \
    do {                                                                                                \
        const _Float16 *krow_ = kb + (size_t)min((KC) * 32 + l31, Tk - 1) * ld + 8 * kh;                \
        _Pragma("unroll") for (int u = 0; u < 8; ++u) {                                                 \
            kh8[u] = *reinterpret_cast<const f16x8 *>(krow_ + 16 * u);                                  \
            kl8[u] = *reinterpret_cast<const f16x8 *>(krow_ + lo_off + 16 * u);                         \
        }                                                                                               \
    } while (0)
#define AX_LOAD_V(KEY0)                                                                                 \
    do {                                                                                                \
        _Pragma("unroll") for (int it = 0; it < 4; ++it) {                                              \
            const int k2_ = min((KEY0) + 4 * it + (lane >> 4), Tk - 1);   /* unit it * 64 + lane = key 4 it + (lane >> 4), channels 8 (lane & 15) .. */ \
            vh8[it] = *reinterpret_cast<const f16x8 *>(vb + (size_t)k2_ * ld + 8 * (lane & 15));       \
            vl8[it] = *reinterpret_cast<const f16x8 *>(vb + (size_t)k2_ * ld + lo_off + 8 * (lane & 15)); \
        }                                                                                               \
    } while (0)
    // 16 keys -> the wave's LDS buffer, row-major
#define AX_STORE_V()                                                                                    \
    do {                                                                                                \
        __builtin_amdgcn_wave_barrier();                                                                \
        _Pragma("unroll") for (int it = 0; it < 4; ++it) {                                              \
            *reinterpret_cast<f16x8 *>(&sVw[(4 * it + (lane >> 4)) * AX_VLD + 8 * (lane & 15)]) = vh8[it]; \
            *reinterpret_cast<f16x8 *>(&sVw[(16 + 4 * it + (lane >> 4)) * AX_VLD + 8 * (lane & 15)]) = vl8[it]; \
        }                                                                                               \
        __builtin_amdgcn_wave_barrier();                                                                \
    } while (0)
    // O^T += V^T P^T over the 16 keys of step S_: per 32-channel block two transposed reads per plane, three MFMAs
#define AX_PV(S_)                                                                                       \
    do {                                                                                                \
        _Pragma("unroll") for (int c = 0; c < NC; ++c) {                                                \
            const _Float16 *t0 = sVw + (4 * kh + ((lane & 15) >> 2)) * AX_VLD + 32 * c + 16 * ((lane >> 4) & 1) + 4 * (lane & 3); \
            const f16x4 h0 = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) atr4 *)(t0))); \
            const f16x4 h1 = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) atr4 *)(t0 + 8 * AX_VLD))); \
            const f16x4 l0 = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) atr4 *)(t0 + 16 * AX_VLD))); \
            const f16x4 l1 = __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) atr4 *)(t0 + 24 * AX_VLD))); \
            const f16x8 ah_ = ax_cat(h0, h1), al_ = ax_cat(l0, l1);                                     \
            o[c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah_, ph[S_], o[c], 0, 0, 0);                  \
            o[c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al_, ph[S_], o[c], 0, 0, 0);                  \
            o[c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah_, pl[S_], o[c], 0, 0, 0);                  \
            if (c & 1) __builtin_amdgcn_sched_barrier(0);   /* (two blocks' operands in flight at a time: registers) */ \
        }                                                                                               \
    } while (0)
    if (kc < nkc) {
        AX_LOAD_K(kc);
        AX_LOAD_V(kc * 32);
    }
    // Q block (rows >= Tq are zeros) -> LDS, shared by the waves: the rows as they are (slot j of step u, half kh = channel 16 u + 8 kh + j)
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const int idx = it * 256 + tid, r = idx >> 4, c8 = 8 * (idx & 15), row = qblk * 32 + r;
        f16x8 qh = {0, 0, 0, 0, 0, 0, 0, 0}, ql = {0, 0, 0, 0, 0, 0, 0, 0};
        if (row < Tq) {
            qh = *reinterpret_cast<const f16x8 *>(qb + (size_t)row * q_ld + c8);
            ql = *reinterpret_cast<const f16x8 *>(qb + (size_t)row * q_ld + lo_off + c8);
        }
        *reinterpret_cast<f16x8 *>(&sQ[r * AX_QLD + c8]) = qh;
        *reinterpret_cast<f16x8 *>(&sQ[(32 + r) * AX_QLD + c8]) = ql;
    }
    __syncthreads();

    f32x16 o[NC];   // o[c][e] on lane (q, half): O[q][32c + (e&3) + 8(e>>2) + 4 half]
    float m_run = -INFINITY, l_run = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[c][e] = 0.f;

    for (; kc < nkc; kc += AX_WAVES) {
        f32x16 sacc;
#pragma unroll
        for (int e = 0; e < 16; ++e) sacc[e] = 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const f16x8 ah = kh8[u], al = kl8[u];
            const f16x8 bh_ = *reinterpret_cast<const f16x8 *>(&sQ[l31 * AX_QLD + u * 16 + kh * 8]);
            const f16x8 bl_ = *reinterpret_cast<const f16x8 *>(&sQ[(32 + l31) * AX_QLD + u * 16 + kh * 8]);
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh_, sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh_, sacc, 0, 0, 0);
            sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl_, sacc, 0, 0, 0);
            if (u & 1) __builtin_amdgcn_sched_barrier(0);   // (two steps' operands at a time: the splits of all eight would not fit the registers)
        }
        // the key rows of this wave's NEXT chunk fly during the softmax and the P V products of this one (their registers are free)
        if (kc + AX_WAVES < nkc) AX_LOAD_K(kc + AX_WAVES);
        // register e = key (e&3) + 8(e>>2) + 4 half of the chunk, for query l31
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const bool kv_ = kc * 32 + (e & 3) + 8 * (e >> 2) + 4 * kh < Tk;
            sacc[e] = kv_ ? sacc[e] * scale : -INFINITY;
            mx = fmaxf(mx, sacc[e]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));          // finite: the chunk has >= 1 valid key
        const float m_new = fmaxf(m_run, mx);
        const float alpha = expf(m_run - m_new);         // exp(-inf) = 0 on the first chunk
        float psum = 0.f;
        f16x8 ph[2], pl[2];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float pe = expf(sacc[e] - m_new);      // exp(-inf) = 0 for keys >= Tk
            psum += pe;
            // P travels as a pair of 2^14 pe: fp16's subnormal spacing makes the pair's quantum ABSOLUTE, 2^-25 for pe itself -- a key with
            // P below that vanished, whatever its value row held -- and 2^-39 for the scaled pe; the merge takes the 2^14 out again (exact)
            const float ps = pe * 16384.f;
            const _Float16 a = (_Float16)ps;               // 0 <= ps <= 16384: no clamp
            ph[e >> 3][e & 7] = a;
            pl[e >> 3][e & 7] = (_Float16)(ps - (float)a);
        }
        l_run = l_run * alpha + psum;
        m_run = m_new;
#pragma unroll
        for (int c = 0; c < NC; ++c)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[c][e] *= alpha;
        AX_STORE_V();
        AX_LOAD_V(kc * 32 + 16);              // the second 16 value rows fly under the first 16 keys' products
        AX_PV(0);
        AX_STORE_V();
        if (kc + AX_WAVES < nkc) AX_LOAD_V((kc + AX_WAVES) * 32);   // ... and the next chunk's first 16 value rows under the second
        AX_PV(1);
        __builtin_amdgcn_wave_barrier();
    }
#undef AX_LOAD_K
#undef AX_LOAD_V
#undef AX_STORE_V
#undef AX_PV

    // ---- merge the 4 waves' partials in wave order (attention_mfma_kernel's): out = sum_w O_w e^(m_w - M) / sum_w l_w e^(m_w - M)
    __syncthreads();   // the merge area aliases the loop's buffers
    float *att_smem = reinterpret_cast<float *>(ax_smem);
    float *sO = att_smem, *sM = att_smem + AX_WAVES * NC * 16 * 64, *sL = sM + AX_WAVES * 32;
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
        for (int w = 1; w < AX_WAVES; ++w) M = fmaxf(M, sM[w * 32 + l31]);
        float a[AX_WAVES], den = 0.f;
#pragma unroll
        for (int w = 0; w < AX_WAVES; ++w) {
            a[w] = expf(sM[w * 32 + l31] - M);   // exp(-inf) = 0 for a wave that had no chunk
            den += sL[w * 32 + l31] * a[w];
        }
        const float inv = 6.103515625e-05f / den;   // 2^-14 / den: O carries the 2^14 of its P pairs, l does not
        const int row = qblk * 32 + l31;
        const int c = wave;   // this wave finishes channel block `wave`
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 r4;
#pragma unroll
            for (int e2 = 0; e2 < 4; ++e2) {
                float num = 0.f;
#pragma unroll
                for (int w = 0; w < AX_WAVES; ++w) num += sO[((w * NC + c) * 16 + 4 * g + e2) * 64 + lane] * a[w];
                r4[e2] = num * inv;
            }
            if (row < Tq) {
                if (pairs) {
                    f16x4 hi4, lo4;
                    // (no range report here: a row is a convex combination of value rows that are pairs already, |r4| <= 65504 up to
                    // rounding -- and a report in this loop changes how the compiler contracts the merge above, i.e. the bits)
                    ax_split4(r4, hi4, lo4);
                    _Float16 *pr = reinterpret_cast<_Float16 *>(out) + (AX_OROW) * (16 * D) + h * D + 32 * c + 8 * g + 4 * kh;
                    *reinterpret_cast<f16x4 *>(pr) = hi4;
                    *reinterpret_cast<f16x4 *>(pr + 8 * D) = lo4;
                } else {
                    *reinterpret_cast<f32x4 *>(out + (AX_OROW) * (8 * D) + h * D + 32 * c + 8 * g + 4 * kh) = r4;
                }
            }
        }
    }
