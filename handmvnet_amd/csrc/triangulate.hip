// Triangulation of the per-view 2D joints (include/handmv.h "triangulation"): one 3D point per (sample, joint) from its V views, by the
// direct linear transform over all usable views or by DLT + RANSAC over a caller-ordered table of camera subsets.
//
// The rule is the reference's utils/triangulation.py -- batch_triangulate_dlt_torch (:99-139) without the + 1e-7 of :137,
// batch_triangulate_dlt_ransac_torch (:5-58) with the candidate order given by the caller, calculate_reprojection_error (:61-95) --
// in fp64 from the fp32 inputs, every operation rounded on its own, outputs rounded once.  Crop-space points are first mapped to the frame
// in fp32, in track.hip's operation order (batch_cropped_joints_to_joints_img, datasets/utils.py:146-162).
//
// The smallest right singular vector of the 2n x 4 DLT matrix A is found without forming A or A^T A: each row is rotated (Givens) into
// a 4x4 upper triangular factor R with R^T R = A^T A, so R has A's right singular vectors and its singular values, and a one-sided Jacobi
// (Hestenes) iteration on R's columns with a fixed number of sweeps finds them.  16 + 16 doubles of state per lane, every index a
// compile-time constant, every loop of the factorisation of constant trip count.
//
// Shaped like pose_consensus.hip: one wave64 per (sample, joint), four per workgroup.  Lanes v < V build the world-to-camera rows W_v and
// the projection matrix M_v = K_v W_v of their view once into LDS -- the cameras of a candidate are named by run-time table entries, and
// a run-time index belongs to LDS, not to a per-lane array -- together with the view's frame-space point.  Lanes stride over the
// candidates, the wave takes the maximum of the key (inliers << 16) | (0xFFFF - s), so the first of the best wins, and the winner's
// point travels by shuffle.  Lanes v < V write the final errors.  No atomics; vector stores in plain C++.  A wave beyond the last row runs
// along on the last row and stores nothing, so the one barrier stays block-wide.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/handmv.h"
#include "kernels.h"

// No a * b + c is contracted into an fma anywhere below, solve4_xyz included.
#pragma clang fp contract(off)
#include "pose_rows.h"

namespace {

constexpr int kWave = 64;
constexpr int kRowsPerBlock = 4;
constexpr int kMaxV = 16;
constexpr int kMaxJ = 64;
constexpr int kMaxS = 4096;
constexpr int kSweeps = 12;   // cyclic Jacobi on a 4x4 converges quadratically; rigs like the fixtures' need 5 (DESIGN.md "Triangulation")

// One row `a` of A into the triangular factor: four Givens rotations, each of row k of R against what is left of `a`.
__device__ __forceinline__ void rotate_in(double R[4][4], double a[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double f = R[k][k], g = a[k];
        const double h = sqrt(f * f + g * g);
        const bool none = h == 0.0;   // (false for a NaN, which then spreads)
        const double c = none ? 1.0 : f / h, s = none ? 0.0 : g / h;
#pragma unroll
        for (int m = k; m < 4; ++m) {
            const double rk = R[k][m], am = a[m];
            R[k][m] = c * rk + s * am;
            a[m] = c * am - s * rk;
        }
    }
}

// The two DLT rows of one view (triangulation.py:128-134): x M[2] - M[0], then y M[2] - M[1].  M: 12 doubles, row-major 3x4.
__device__ __forceinline__ void add_view(double R[4][4], const double *M, double x, double y) {
    double a[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) a[c] = x * M[8 + c] - M[c];
    rotate_in(R, a);
#pragma unroll
    for (int c = 0; c < 4; ++c) a[c] = y * M[8 + c] - M[4 + c];
    rotate_in(R, a);
}

__device__ __forceinline__ void clear(double R[4][4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) R[i][k] = 0.0;
}

// X = v[:3] / v[3], v the right singular vector of R's smallest singular value: one-sided Jacobi on the columns of R (overwritten),
// kSweeps sweeps over the six column pairs, a pair that is orthogonal to working precision left alone (svd3's test, pose_rows.h).
__device__ __forceinline__ void null_point(double W[4][4], double X[3]) {
    double Vm[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) Vm[i][k] = i == k ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kSweeps; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    al += W[i][p] * W[i][p];
                    be += W[i][q] * W[i][q];
                    ga += W[i][p] * W[i][q];
                }
                const bool skip = fabs(ga) <= 1e-300 || fabs(ga) <= 1e-17 * sqrt(al * be);
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cr = 1.0 / sqrt(1.0 + t * t);
                const double c = skip ? 1.0 : cr, sn = skip ? 0.0 : cr * t;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const double wp = W[i][p], wq = W[i][q];
                    W[i][p] = c * wp - sn * wq;
                    W[i][q] = sn * wp + c * wq;
                    const double vp = Vm[i][p], vq = Vm[i][q];
                    Vm[i][p] = c * vp - sn * vq;
                    Vm[i][q] = sn * vp + c * vq;
                }
            }
    }
    double best = 0.0, v[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double n = ((W[0][k] * W[0][k] + W[1][k] * W[1][k]) + W[2][k] * W[2][k]) + W[3][k] * W[3][k];
        if (k == 0 || n < best) {
            best = n;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = Vm[i][k];
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) X[c] = v[c] / v[3];
}

// The reprojection error of X in one view (calculate_reprojection_error, :79-88): |point - (M [X; 1])[:2] / (M [X; 1])[2]|.
__device__ __forceinline__ double reprojection_error(const double *M, double x, double y, const double X[3]) {
    double h[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) h[r] = ((M[r * 4] * X[0] + M[r * 4 + 1] * X[1]) + M[r * 4 + 2] * X[2]) + M[r * 4 + 3];
    const double dx = x - h[0] / h[2], dy = y - h[1] / h[2];
    return sqrt(dx * dx + dy * dy);
}

// The DLT over the views of `mask`, ascending.
__device__ __forceinline__ void dlt_views(const double (*M)[12], const double (*P)[2], unsigned mask, int V, double X[3]) {
    double R[4][4];
    clear(R);
    for (int v = 0; v < V; ++v)
        if ((mask >> v) & 1u) add_view(R, M[v], P[v][0], P[v][1]);
    null_point(R, X);
}

// fp32, each operation rounded on its own (the file is compiled without contraction): track.hip's forms of the same mapping
__device__ __forceinline__ float mul_rn(float x, float y) { return x * y; }
__device__ __forceinline__ float add_rn(float x, float y) { return x + y; }
__device__ __forceinline__ float sub_rn(float x, float y) { return x - y; }
__device__ __forceinline__ float div_rn(float x, float y) { return x / y; }

__global__ __launch_bounds__(kWave * kRowsPerBlock) void triangulate_kernel(const hmv::TriangulateParams p) {
    __shared__ double sM[kRowsPerBlock][kMaxV][12];   // K W: the projection matrices
    __shared__ double sW[kRowsPerBlock][kMaxV][12];   // rows 0..2 of world-to-camera
    __shared__ double sP[kRowsPerBlock][kMaxV][2];    // the view's point in frame pixels
    const int lane = (int)threadIdx.x & (kWave - 1), w = (int)threadIdx.x >> 6;
    const long total = (long)p.B * p.J;
    long row = (long)blockIdx.x * kRowsPerBlock + w;
    const bool valid = row < total;
    if (!valid) row = total - 1;
    const long b = row / p.J;
    const int j = (int)(row - b * p.J);
    const int V = p.V;

    bool usable = false;
    if (lane < V) {
        const long bv = b * V + lane;
        const float *e = p.extrinsic + bv * 16;
        double W[3][4];
        if (p.kind == 0) {
            inverse_rows(e, W);
        } else {
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) W[r][c] = (double)e[r * 4 + c];
        }
        const double fx = (double)p.intrinsic[bv * 4], fy = (double)p.intrinsic[bv * 4 + 1];
        const double cx = (double)p.intrinsic[bv * 4 + 2], cy = (double)p.intrinsic[bv * 4 + 3];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            sM[w][lane][c] = fx * W[0][c] + cx * W[2][c];
            sM[w][lane][4 + c] = fy * W[1][c] + cy * W[2][c];
            sM[w][lane][8 + c] = W[2][c];
#pragma unroll
            for (int r = 0; r < 3; ++r) sW[w][lane][r * 4 + c] = W[r][c];
        }
        float x = p.points[(bv * p.J + j) * 2], y = p.points[(bv * p.J + j) * 2 + 1];
        if (p.bbox) {   // batch_cropped_joints_to_joints_img in its own operation order
            const float *box = p.bbox + bv * 4;
            const float S = (float)p.image_size;
            const float x1f = box[0], y1f = box[1];
            const float wf = sub_rn(box[2], x1f), hf = sub_rn(box[3], y1f);
            x = add_rn(mul_rn(x, div_rn(wf, S)), x1f);
            y = add_rn(mul_rn(y, div_rn(hf, S)), y1f);
        }
        sP[w][lane][0] = (double)x;
        sP[w][lane][1] = (double)y;
        usable = (!p.present || p.present[bv] != 0) && (!p.joint_mask || p.joint_mask[bv * p.J + j] == 0);
    }
    const unsigned umask = (unsigned)__ballot(usable);
    const int n_usable = __popc(umask);
    __syncthreads();

    const double (*M)[12] = sM[w];
    const double (*P)[2] = sP[w];
    const double nan = (double)NAN;
    double X[3] = {nan, nan, nan};
    int key = -1;   // (inliers << 16) | (0xFFFF - s) of this lane's best candidate; -1: none
    if (n_usable >= 2) {
        if (!p.subsets) {   // every lane the same DLT
            dlt_views(M, P, umask, V, X);
            key = 0;
        } else {
            for (int s = lane; s < p.S; s += kWave) {
                const int *cams = p.subsets + (long)s * p.n_cams;
                bool ok = true;
                for (int i = 0; i < p.n_cams; ++i) {
                    const int c = cams[i];
                    ok = ok && c >= 0 && c < V && ((umask >> (c & (kMaxV - 1))) & 1u);
                }
                if (!ok) continue;   // names a camera outside [0, V) or one that is not usable: skipped, nothing is indexed by it
                double R[4][4];
                clear(R);
                for (int i = 0; i < p.n_cams; ++i) {
                    const int c = cams[i];
                    add_view(R, M[c], P[c][0], P[c][1]);
                }
                double Y[3];
                null_point(R, Y);
                int n = 0;
                for (int v = 0; v < V; ++v)
                    if ((umask >> v) & 1u) n += reprojection_error(M[v], P[v][0], P[v][1], Y) < p.threshold ? 1 : 0;
                const int k = (n << 16) | (0xFFFF - s);
                if (k > key) {
                    key = k;
                    X[0] = Y[0]; X[1] = Y[1]; X[2] = Y[2];
                }
            }
        }
    }
    int best = key;
    for (int m = kWave / 2; m >= 1; m >>= 1) best = max(best, __shfl_xor(best, m, kWave));
    const int owner = __ffsll((unsigned long long)__ballot(key == best)) - 1;   // keys of candidates are distinct; all -1: lane 0's NaN
#pragma unroll
    for (int c = 0; c < 3; ++c) X[c] = __shfl(X[c], owner, kWave);

    int st = 0, win = -1, n_inl = 0;
    if (best < 0) {
        st = 2;
    } else if (p.subsets) {
        n_inl = best >> 16;
        if (n_inl == 0) {
            st = 1;
            X[0] = X[1] = X[2] = 0.0;
        } else {
            win = 0xFFFF - (best & 0xFFFF);
            const int v = lane < V ? lane : 0;
            const bool in = lane < V && usable && reprojection_error(M[v], P[v][0], P[v][1], X) < p.threshold;
            const unsigned imask = (unsigned)__ballot(in);
            if (p.refit && __popc(imask) >= 2) dlt_views(M, P, imask, V, X);
        }
    } else {
        n_inl = n_usable;
    }

    if (p.reproj_err && valid && lane < V) {
        const double err = reprojection_error(M[lane], P[lane][0], P[lane][1], X);
        p.reproj_err[(b * V + lane) * p.J + j] = usable ? (float)err : NAN;
    }
    float o[3] = {(float)X[0], (float)X[1], (float)X[2]};
    if (p.frame_cam && st == 0) {
        const int fc = p.frame_cam[b];
        const bool bad = fc < 0 || fc >= V;
        const double *Wc = sW[w][bad ? 0 : fc];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double y = ((Wc[r * 4] * X[0] + Wc[r * 4 + 1] * X[1]) + Wc[r * 4 + 2] * X[2]) + Wc[r * 4 + 3];
            o[r] = bad ? NAN : (float)y;
        }
    }
    if (st == 0 && !(isfinite(o[0]) && isfinite(o[1]) && isfinite(o[2]))) st = 3;
    if (valid && lane == 0) {
        float *out = p.points3d + row * 3;
        out[0] = o[0]; out[1] = o[1]; out[2] = o[2];
        p.status[row] = st;
        if (p.inliers) p.inliers[row] = n_inl;
        if (p.winner) p.winner[row] = win;
    }
}

using hmv::bad_arg;
using hmv::hip_fail;

}  // namespace

namespace hmv {

hipError_t launch_triangulate(const TriangulateParams &p, hipStream_t s) {
    const long rows = (long)p.B * p.J;
    const unsigned blocks = (unsigned)((rows + kRowsPerBlock - 1) / kRowsPerBlock);
    hipLaunchKernelGGL(triangulate_kernel, dim3(blocks), dim3(kWave * kRowsPerBlock), 0, s, p);
    return hipGetLastError();
}

}  // namespace hmv

extern "C" int hmv_op_triangulate(int32_t device, const hmv_triangulate_args *a, void *stream) {
    const char *who = "hmv_op_triangulate";
    if (!a) return bad_arg(who, "args is NULL");
    if (a->struct_size != (int32_t)sizeof(hmv_triangulate_args)) return bad_arg(who, "struct_size does not match this library's hmv_triangulate_args");
    if (a->B < 1) return bad_arg(who, "B must be >= 1");
    if (a->V < 1 || a->V > kMaxV) return bad_arg(who, "V must be in 1 .. 16");
    if (a->J < 1 || a->J > kMaxJ) return bad_arg(who, "J must be in 1 .. 64");
    if ((int64_t)a->B * a->J > (1 << 24)) return bad_arg(who, "B * J must not exceed 2^24 points");
    if (!a->points) return bad_arg(who, "points is NULL");
    if (!a->intrinsic) return bad_arg(who, "intrinsic is NULL");
    if (!a->extrinsic) return bad_arg(who, "extrinsic is NULL");
    if (!a->points3d) return bad_arg(who, "points3d is NULL");
    if (!a->status) return bad_arg(who, "status is NULL");
    if (a->extrinsic_kind != 0 && a->extrinsic_kind != 1) return bad_arg(who, "extrinsic_kind must be 0 (camera-to-world) or 1 (world-to-camera)");
    if (a->bbox && a->image_size < 1) return bad_arg(who, "image_size must be >= 1 when bbox is given");
    if (a->subsets) {
        if (a->S < 1 || a->S > kMaxS) return bad_arg(who, "S must be in 1 .. 4096 when subsets is given");
        if (a->n_cams < 2 || a->n_cams > a->V) return bad_arg(who, "n_cams must be in 2 .. V when subsets is given");
        if (!(a->threshold > 0.f) || !isfinite(a->threshold)) return bad_arg(who, "threshold must be finite and > 0 when subsets is given");
    }
    if (a->refit != 0 && a->refit != 1) return bad_arg(who, "refit must be 0 or 1");
    if (hipSetDevice(device) != hipSuccess) return hip_fail(who, hipGetLastError());
    const bool table = a->subsets != nullptr;
    const hmv::TriangulateParams p{a->points, a->bbox, a->intrinsic, a->extrinsic, a->present, a->joint_mask, a->subsets, a->frame_cam,
                                   a->B, a->V, a->J, table ? a->S : 0, table ? a->n_cams : 0, a->image_size, a->extrinsic_kind,
                                   table ? a->refit : 0, table ? (double)a->threshold : 0.0,
                                   a->points3d, a->reproj_err, a->inliers, a->winner, a->status};
    const hipError_t e = hmv::launch_triangulate(p, (hipStream_t)stream);
    return e == hipSuccess ? HMV_OK : hip_fail(who, e);
}
