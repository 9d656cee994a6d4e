// The per-segment moments of phgpu_gap_moments (included by phgpu.hip; DESIGN.md 3.20): what the
// Mak-Morton-Wood gap estimator and zhat4xhat need of two batched solves
// (confidence_intervals/ciutils.py:400-415 gathers them scenario by scenario on the host).
//
// One lane per local scenario.  The segments are ascending ranges of global scenario indices,
// so a wave's lanes carry non-decreasing segment keys and every segment is ONE run of lanes in
// each wave it touches.  k_gap_partial sums every run by a segmented scan (shuffles, fixed
// order) and its last lane stores the sum: a run that touches neither end of the wave is a
// whole segment and goes straight to its row of out; the run at lane 0 (head) and the run at
// lane 63 (tail) may continue in the neighbouring waves and go to the wave's two slots of the
// workspace, tagged by segment.  k_gap_final, one wave per segment, adds the slots of the
// segment's waves in wave order.  No atomics: two calls give the same bits.

#define GM_NV 7   // sum p, p^2, p g, p g^2, p f_hat, p f_star, scenarios left out
#define GM_ROW 8  // doubles per row of out (entry 7 is 0)

// the segment of global scenario g: the last j with seg_ptr[j] <= g; -1 ahead of the first
// segment, nseg behind the last one
__device__ __forceinline__ int gm_segment(const int64_t* __restrict__ seg_ptr, int nseg, int64_t g) {
    if (g < seg_ptr[0]) return -1;
    int lo = 0, hi = nseg;  // seg_ptr[lo] <= g, and g < seg_ptr[hi + 1] or hi == nseg
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_ptr[mid] <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__global__ void __launch_bounds__(BLOCK)
k_gap_partial(ph_tree st, const double* __restrict__ f_hat, const int32_t* __restrict__ st_hat,
              const double* __restrict__ f_star, const int32_t* __restrict__ st_star,
              const int64_t* __restrict__ seg_ptr, int nseg, int64_t s_off, double* __restrict__ part,
              int32_t* __restrict__ tag, double* __restrict__ out) {
    const int64_t S = st.S;
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t wave = s / WAVE;
    double v[GM_NV];
#pragma unroll
    for (int j = 0; j < GM_NV; ++j) v[j] = 0.0;
    int key = nseg + 1;  // a lane past the local scenarios
    if (s < S) {
        key = gm_segment(seg_ptr, nseg, s_off + s);
        const bool ok = st_hat[s] == PHGPU_OPTIMAL && (!st_star || st_star[s] == PHGPU_OPTIMAL);
        if (ok) {
            const double p = st.prob[s], fh = f_hat[s], fs = f_star ? f_star[s] : 0.0;
            const double g = f_star ? fh - fs : 0.0;
            v[0] = p;
            v[1] = p * p;
            v[2] = p * g;
            v[3] = p * g * g;
            v[4] = p * fh;
            v[5] = p * fs;
        } else {
            v[6] = 1.0;
        }
    }
    // segmented inclusive scan: after it the last lane of a run holds the run's sum
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const int ku = __shfl_up(key, off, WAVE);
        const bool take = lane >= off && ku == key;
#pragma unroll
        for (int j = 0; j < GM_NV; ++j) {
            const double u = __shfl_up(v[j], off, WAVE);
            v[j] += take ? u : 0.0;
        }
    }
    const int key0 = __shfl(key, 0, WAVE), key63 = __shfl(key, WAVE - 1, WAVE);
    const int knext = __shfl_down(key, 1, WAVE);
    const bool last = lane == WAVE - 1 || knext != key;
    if (!last) return;
    if (key == key0) {  // the head run (the whole wave when it reaches lane 63)
#pragma unroll
        for (int j = 0; j < GM_NV; ++j) part[(wave * 2 + 0) * GM_NV + j] = v[j];
        tag[wave * 2 + 0] = key;
        if (lane == WAVE - 1) tag[wave * 2 + 1] = -1;
    } else if (key == key63) {  // the tail run
#pragma unroll
        for (int j = 0; j < GM_NV; ++j) part[(wave * 2 + 1) * GM_NV + j] = v[j];
        tag[wave * 2 + 1] = key;
    } else if (key >= 0 && key < nseg) {  // a whole segment inside the wave
#pragma unroll
        for (int j = 0; j < GM_NV; ++j) out[(int64_t)key * GM_ROW + j] = v[j];
        out[(int64_t)key * GM_ROW + GM_NV] = 0.0;
    }
}

// One wave per segment: the rows the partial pass did not store.  A segment without local
// scenarios gets zeros; the others the head / tail slots that carry their tag, lane l taking
// the waves w0 + l, w0 + l + 64, .. in order, then the fixed-order wave sum.
__global__ void __launch_bounds__(WAVE)
k_gap_final(int64_t S, const int64_t* __restrict__ seg_ptr, int64_t s_off, const double* __restrict__ part,
            const int32_t* __restrict__ tag, double* __restrict__ out) {
    const int j = blockIdx.x;
    const int lane = threadIdx.x;
    int64_t a = seg_ptr[j] - s_off, b = seg_ptr[j + 1] - s_off;
    a = a < 0 ? 0 : a;
    b = b > S ? S : b;
    double v[GM_NV];
#pragma unroll
    for (int t = 0; t < GM_NV; ++t) v[t] = 0.0;
    if (a < b) {
        const int64_t w0 = a / WAVE, w1 = (b - 1) / WAVE;
        if (w0 == w1 && a % WAVE != 0 && b % WAVE != 0) return;  // stored by the partial pass
        for (int64_t w = w0 + lane; w <= w1; w += WAVE) {
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                if (tag[w * 2 + side] != j) continue;
#pragma unroll
                for (int t = 0; t < GM_NV; ++t) v[t] += part[(w * 2 + side) * GM_NV + t];
            }
        }
#pragma unroll
        for (int t = 0; t < GM_NV; ++t) v[t] = wave_sum(v[t]);
    }
    if (lane == 0) {
#pragma unroll
        for (int t = 0; t < GM_NV; ++t) out[(int64_t)j * GM_ROW + t] = v[t];
        out[(int64_t)j * GM_ROW + GM_NV] = 0.0;
    }
}
