// The body of the epoch kernels (eval_epoch.hip), shared as TEXT by eval_epoch_kernel and eval_epoch_views_kernel so that the two have
// one copy of the arithmetic and the uniform kernel's device code stays what it was (tools/isa_diff.py).  In scope: a (EpochParams).
// The including kernel defines
//   EPOCH_PROLOGUE            statements after the LDS declarations (the ragged kernel counts each sample's present views there)
//   EPOCH_2D_ROW(r)           statements at the top of the 2D loop's body for row r; may `continue` (an absent row is not read)
//   EPOCH_2D_TERM(dist)       what row r adds to the 2D sum for its distance `dist` (a double)
    __shared__ double red[kThreads];
    __shared__ float thr[kMaxSteps];
    __shared__ int hist[kMaxSteps + 1];
    const int t = threadIdx.x;
    EPOCH_PROLOGUE
    fill_thresholds(thr, a.tmin, a.tmax, a.steps);
    if (t <= a.steps) hist[t] = 0;
    __syncthreads();

    // ---- the 3D distances that remain after the similarity alignment of each pose, one lane per pose.  First, while nothing else
    // is live: the alignment needs every register a lane has
    double acc = 0.0;
    for (int first = 0; first < a.B; first += kThreads) {   // a uniform counter: the lane keeps no loop state of its own
        const int sidx = first + t;
        if (sidx >= a.B) continue;
        const float *p = a.pred_cam + (long)sidx * NJ * 3;
        const float *g = a.gt_cam + (long)sidx * NJ * 3;
        float *const no_output = nullptr;
        double U[3][3], S[3], V[3][3];
        {
            POSE_MOMENTS(p, g, a.n_pts, mu1, mu2, var1, K)
            svd3(K, U, S, V);
            (void)var1;
        }
        // the moments again rather than kept: with them live across svd3 the lane's working set does not fit the 128 registers a
        // 1024-lane workgroup leaves it
        POSE_MOMENTS(p, g, a.n_pts, mu1, mu2, var1, K)
        POSE_ADD_ALIGNED_ERROR(p, g, a.n_pts, mu1, mu2, var1, K, U, V, no_output, 0L, acc)
    }
    const double sum_pa = block_sum(acc, red);

    // ---- 3D: joint distances and their PCK bins
    const long rows3 = (long)a.B * NJ;
    acc = 0.0;
    for (long r = t; r < rows3; r += kThreads) {
        const float dist = row_distance(a.pred_cam + r * 3, a.gt_cam + r * 3, 3);
        acc += (double)dist;
        atomicAdd(&hist[threshold_bin(dist, thr, a.steps)], 1);
    }
    const double sum3 = block_sum(acc, red);

    // ---- 2D: masked joints are zeroed on both sides (models/utils.py:123-131), so they add 0 and still count
    const long rows2 = (long)a.B * a.V * NJ;
    acc = 0.0;
    for (long r = t; r < rows2; r += kThreads) {
        EPOCH_2D_ROW(r)
        const float keep = (a.mask && a.mask[r]) ? 0.f : 1.f;
        const float p[2] = {a.pred_2d[r * 2] * keep, a.pred_2d[r * 2 + 1] * keep};
        const float g[2] = {a.gt_2d[r * 2] * keep, a.gt_2d[r * 2 + 1] * keep};
        acc += EPOCH_2D_TERM((double)row_distance(p, g, 2));
    }
    const double sum2 = block_sum(acc, red);   // its leading barrier also completes hist

    if (t == 0) {
        double *s = a.state;
        s[0] += (double)a.B;
        s[1] += 1.0;
        s[2] += (double)rows3;
        s[3] += sum3;
        s[4] += sum_pa;
        s[5] += (double)rows2;
        s[6] += sum2;
        if (a.loss) {
            s[7] += (double)a.B;
            for (int i = 0; i < 6; ++i) s[8 + i] += (double)a.B * (double)a.loss[i];
        }
        for (int i = 0; i <= a.steps; ++i) s[kScalars + i] += (double)hist[i];
    }
