// Body of tokens_finalize_kernel and tokens_finalize_views_kernel (misc_kernels.hip), included once by each: the two differ only in
// TOK_POS, the position of row (frame n, joint j) inside its sample.  Textual sharing, so that the uniform kernel's code is the
// compiler's output for exactly the token sequence it always had.
    const int row = blockIdx.x;           // n*21 + j, n = b*V + v
    const int n = row / 21, j = row - n * 21;
    float *t = tokens + (size_t)row * ldt;
    int col = fdim;
    if (threadIdx.x == 0) {
        if (pos_mask & 1) { t[col] = coords[2 * row]; t[col + 1] = coords[2 * row + 1]; }
    }
    if (pos_mask & 1) col += 2;
    if ((pos_mask & 2) && threadIdx.x < 10) {
        const float *bb = bbox + 4 * n, *in = intr + 4 * n;
        const int pt = threadIdx.x >> 1, isy = threadIdx.x & 1;
        float px, py;
        if (pt == 0) { px = bb[0]; py = bb[1]; }
        else if (pt == 1) { px = bb[0]; py = bb[3]; }
        else if (pt == 2) { px = bb[2]; py = bb[1]; }
        else if (pt == 3) { px = bb[2]; py = bb[3]; }
        else { px = (bb[0] + bb[2]) / 2.f; py = (bb[1] + bb[3]) / 2.f; }
        t[col + threadIdx.x] = isy ? atanf((py - in[3]) / in[1]) : atanf((px - in[2]) / in[0]);
    }
    for (int c = d + threadIdx.x; c < ldt; c += blockDim.x) t[c] = 0.f;
    __syncthreads();
    const int pos = TOK_POS;  // token index inside its sample, view-major
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        float v = t[c];
        if (raw_copy) raw_copy[(size_t)row * d + c] = v;
        if (pe) { v = v + pe[(size_t)pos * d + c]; t[c] = v; }
        if (pairs) {
            _Float16 a, b;
            note_range(sat, split_f16(v, a, b));
            pairs[(size_t)row * 2 * ldt + c] = a;
            pairs[(size_t)row * 2 * ldt + ldt + c] = b;
        }
    }
    if (pairs)
        for (int c = d + threadIdx.x; c < ldt; c += blockDim.x) { pairs[(size_t)row * 2 * ldt + c] = (_Float16)0.f; pairs[(size_t)row * 2 * ldt + ldt + c] = (_Float16)0.f; }
