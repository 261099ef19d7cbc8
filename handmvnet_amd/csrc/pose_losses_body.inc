// The body of the first launch of the loss entries (losses.hip), shared as TEXT by pose_losses_kernel and pose_losses_views_kernel
// so that the two have one copy of the arithmetic and the uniform kernel's device code stays what it was (tools/isa_diff.py).
// In scope: pred, target, labels, S, h, w, sigma, partial (the kernel's parameters), f (frame slot), t (lane), lds (the reduction
// buffer, kThreads doubles) and prof (the profile area behind it).
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
    const double s = block_sum(acc, lds);
    if (t == 0) partial[f] = s;
