// The frame-preparation kernels (misc_kernels.hip), shared as TEXT by the plain and the indexed (ragged view sets) forms, so that both
// have one copy of the addressing and the plain kernels' device code stays what it was (tools/isa_diff.py).  The including file defines
//   FRAMES_TO_INPUT_KERNEL / FRAMES_TO_S2D_KERNEL   the kernels' names
//   FRAMES_EXTRA_PARAMS                             parameters behind `boxes` (with their trailing comma), or nothing
//   FRAME_PIXEL(n, oy, ox, r, g, b)                 output pixel (oy, ox) of OUTPUT frame n into the floats r, g, b
// OUT: 0 = NHWC4 fp32, 1 = NHWC8 fp16, 2 = split [hi8 | lo8] fp16 pairs (HMV_F32X3)
template <int OUT>
__global__ void FRAMES_TO_INPUT_KERNEL(const uint8_t *__restrict__ frames, const int *__restrict__ boxes, FRAMES_EXTRA_PARAMS int Hf, int Wf, int S_h,
                                       int S_w, FrameNorm nm, void *__restrict__ out, size_t total) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        const int ox = (int)(i % S_w);
        size_t t = i / S_w;
        const int oy = (int)(t % S_h);
        const size_t n = t / S_h;
        float r, g, b;
        FRAME_PIXEL(n, oy, ox, r, g, b);
        if (OUT == 2) {
            f16x8 hv = {0, 0, 0, 0, 0, 0, 0, 0}, lv = {0, 0, 0, 0, 0, 0, 0, 0};
            _Float16 a, c;
            split_f16(r, a, c); hv[0] = a; lv[0] = c;
            split_f16(g, a, c); hv[1] = a; lv[1] = c;
            split_f16(b, a, c); hv[2] = a; lv[2] = c;
            reinterpret_cast<f16x8 *>(out)[2 * i] = hv;
            reinterpret_cast<f16x8 *>(out)[2 * i + 1] = lv;
        } else if (OUT == 1) {
            f16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
            v[0] = (_Float16)r; v[1] = (_Float16)g; v[2] = (_Float16)b;
            reinterpret_cast<f16x8 *>(out)[i] = v;
        } else {
            reinterpret_cast<f32x4 *>(out)[i] = f32x4{r, g, b, 0.f};
        }
    }
}
// the same into the space-to-depth stem layout (nchw_to_s2d_kernel above): one thread per s2d pixel = 2 x 2 output pixels
template <int MODE>
__global__ void FRAMES_TO_S2D_KERNEL(const uint8_t *__restrict__ frames, const int *__restrict__ boxes, FRAMES_EXTRA_PARAMS int Hf, int Wf, int S_h,
                                     int S_w, int Hs, int Ws, FrameNorm nm, void *__restrict__ out, size_t total) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        const int xs = (int)(i % Ws);
        size_t t = i / Ws;
        const int ys = (int)(t % Hs);
        const size_t n = t / Hs;
        float v[12];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const int oy = 2 * ys + dy, ox = 2 * xs + dx, j = (dy * 2 + dx) * 3;
                v[j] = v[j + 1] = v[j + 2] = 0.f;
                if (oy < S_h && ox < S_w) FRAME_PIXEL(n, oy, ox, v[j], v[j + 1], v[j + 2]);
            }
        s2d_store<MODE>(out, i, v);
    }
}
