// pxl_baseline.h -- the two passes of the destriping map-maker over one time chunk of a (D, T) observation with nearest-pixel
// (order 0) polarised pointing: binning a timestream with its baselines removed, and projecting a timestream
// with the sky removed back onto the baselines; included by pxl_kernels.hip after pxl_nearest.h (one translation unit,
// -ffp-contract=off).
//
// A chunk is detector-major as k_pointing_expand writes it: N = n_det * n_chunk samples, sample k has det = k / n_chunk and
// j = k % n_chunk, its time is t0 + j and its baseline b = det * n_base + (t0 + j) / baseline_len.  Both kernels form the pixel
// with cell0<true> exactly as k_bin_pol_nearest does, and share baseline_value and baseline_live below, so a sample one of them
// cuts is a sample the other cuts.

// ---- the sample value: d_k (a null), a[b] (d null), d_k - a[b] with one rounding (both given).  ab: a[b] as the caller loaded
// it (anything where a is null); d is read only where there is one.
__device__ __forceinline__ double baseline_value(const double* __restrict__ d, const double* __restrict__ a, int64_t k, double ab) {
    if (!a) return d[k];
    if (!d) return ab;
    return d[k] - ab;
}
// ---- a sample is cut where it has no pixel (off the map, a position that is not finite, past the batch) or its pixel's mask
// value is not > 0 (NaN included).  `m` is what load0 read at the pixel; a null mask keeps everything.
__device__ __forceinline__ bool baseline_live(const Cell0& c, bool masked, double m) {
    return c.off >= 0 && (!masked || m > 0.0);
}
// t / len for 0 <= t: a 32-bit division where the caller knows every time of the chunk fits one
__device__ __forceinline__ int64_t baseline_div(int64_t t, int64_t len, bool small) {
    return small ? (int64_t)((uint32_t)t / (uint32_t)len) : t / len;
}

// ---- bin: rhs3 += P^T (w o x) over the uncut samples.  v = w[k] * x_k with one rounding, then what k_scatter_pol_nearest<3> adds
// for v: the same multiset of terms, bit for bit, as that scatter of the products restricted to the uncut samples.  Full maps
// only.  A cut sample's d and a are not read into the sum at all: a NaN there stays out of the map.
__global__ __launch_bounds__(256) void k_baseline_bin(Sky2Pix s, double* __restrict__ rhs3, const double* __restrict__ mask,
                                                      int64_t nx, int64_t ny, int periodic, int64_t n, int64_t n_chunk, int64_t t0,
                                                      int64_t len, int64_t n_base, int small, const double2* __restrict__ sky,
                                                      const double2* __restrict__ resp, const double* __restrict__ w,
                                                      const double* __restrict__ d, const double* __restrict__ a) {
    const int64_t plane = nx * ny;
    for (Trip<PXL_ZUNR> trip; trip.k0 < n; trip.next()) {
        double2 ad[PXL_ZUNR], qu[PXL_ZUNR];
        double xk[PXL_ZUNR], wk[PXL_ZUNR];
        trip.load(sky, n, ad, make_double2(0.0, 0.0));
        trip.load(resp, n, qu, make_double2(0.0, 0.0));
        trip.load(w, n, wk, 0.0);
#pragma unroll
        for (int u = 0; u < PXL_ZUNR; ++u) {
            const int64_t k = trip.k(u);
            xk[u] = 0.0;
            if (k < n) {
                const int64_t det = small ? (int64_t)((uint32_t)k / (uint32_t)n_chunk) : k / n_chunk;
                const int64_t b = det * n_base + baseline_div(t0 + (k - det * n_chunk), len, small);
                xk[u] = baseline_value(d, a, k, a ? a[b] : 0.0);
            }
        }
        Cell0 cell[PXL_ZUNR];
        double mk[PXL_ZUNR];
#pragma unroll
        for (int u = 0; u < PXL_ZUNR; ++u) cell[u] = cell0<true>(s, ad[u], nx, ny, 0, ny, periodic, trip.k(u) < n);
#pragma unroll
        for (int u = 0; u < PXL_ZUNR; ++u) mk[u] = mask ? load0(mask, cell[u], sky) : 1.0;
#pragma unroll
        for (int u = 0; u < PXL_ZUNR; ++u) {
            if (!baseline_live(cell[u], mask != nullptr, mk[u])) continue;
            const double v = wk[u] * xk[u];
            double t[3];
            pol_terms<3>(v, qu[u], t);
#pragma unroll
            for (int c = 0; c < 3; ++c) scatter_add(rhs3 + (int64_t)c * plane + cell[u].off, t[c]);
        }
    }
}

// ---- project: out[b] += sum over the uncut samples k of baseline b in this chunk of w_k * (x_k - s_k), s_k = (s_I + q_k s_Q) +
// u_k s_U of map3 at the sample's pixel (k_sample_pol_nearest's operations in its order); with a null map3 the term is w_k * x_k.
//
// No atomics.  A SEGMENT is one detector's samples of one baseline inside the chunk; the chunk has n_det * nseg of them, nseg the
// baselines [b_lo, b_lo + nseg) the chunk's times meet.  A segment is summed by ONE group of G lanes (G a power of two, 1 to 256,
// chosen by the host from baseline_len alone): lane l adds the terms of the uncut samples j = lo + l, lo + l + G, ... in that
// order into its own sum starting from +0.0, the lane sums are joined by a fixed tree (shuffles within a wavefront:
// l += l + G/2, ..., l += l + 1; for G = 256 the four wavefronts' sums through LDS as (s0 + s1) + (s2 + s3)), and lane 0 does
// out[b] = out[b] + sum with a plain load and store -- only if the segment had an uncut sample, so a baseline whose samples
// here are all cut keeps its bits.  No two segments of one launch share a baseline, so nothing races, and the bits depend on
// the arguments alone.  A group of G < 64 lanes shares its wavefront with 64 / G - 1 other segments: that is how short
// baselines are packed.  U: samples per lane and trip whose loads are issued together; it does not change the order of a sum.
template <int U>
__global__ __launch_bounds__(256) void k_baseline_project(Sky2Pix s, const double* __restrict__ map3, const double* __restrict__ mask,
                                                          int64_t nx, int64_t ny, int periodic, int64_t n_chunk, int64_t t0,
                                                          int64_t len, int64_t n_base, int64_t b_lo, int64_t nseg, int64_t nseg_all,
                                                          int G, const double2* __restrict__ sky, const double2* __restrict__ resp,
                                                          const double* __restrict__ w, const double* __restrict__ d,
                                                          const double* __restrict__ a, double* __restrict__ out) {
    __shared__ double wave_sum[4];
    __shared__ int wave_hit[4];
    const int64_t plane = nx * ny;
    const int gpb = 256 / G;                                    // groups (segments) per block and trip
    const int lane = threadIdx.x & (G - 1);
    // every lane of a block makes the same number of trips: the shuffles and the barriers below are never divergent
    for (int64_t seg0 = (int64_t)blockIdx.x * gpb; seg0 < nseg_all; seg0 += (int64_t)gridDim.x * gpb) {
        const int64_t seg = seg0 + threadIdx.x / G;
        const bool has = seg < nseg_all;
        const int64_t det = has ? seg / nseg : 0;
        const int64_t brel = b_lo + (has ? seg - det * nseg : 0);          // the baseline's index within its detector
        const int64_t b = det * n_base + brel;
        // the segment's samples: j in [lo, hi) of the chunk (empty for a group past the last segment)
        const int64_t first = brel * len;                                  // the baseline's own times are [first, first + len)
        const int64_t lo = has ? (first > t0 ? first - t0 : 0) : 0;
        const int64_t hi = has ? (t0 + n_chunk - first > len ? first + len - t0 : n_chunk) : 0;
        const double ab = (has && a) ? a[b] : 0.0;
        const int64_t k_det = det * n_chunk;
        double acc = 0.0;
        int hit = 0;
        for (int64_t j0 = lo + lane; j0 < hi; j0 += (int64_t)G * U) {
            double2 ad[U], qu[U];
            double xk[U], wk[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t j = j0 + (int64_t)u * G;
                const bool in = j < hi;
                const int64_t k = k_det + j;
                ad[u] = in ? sky[k] : make_double2(0.0, 0.0);
                qu[u] = in ? resp[k] : make_double2(0.0, 0.0);
                wk[u] = in ? w[k] : 0.0;
                xk[u] = in ? baseline_value(d, a, k, ab) : 0.0;
            }
            Cell0 cell[U];
            double mk[U], v[U][3];
#pragma unroll
            for (int u = 0; u < U; ++u) cell[u] = cell0<true>(s, ad[u], nx, ny, 0, ny, periodic, j0 + (int64_t)u * G < hi);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                mk[u] = mask ? load0(mask, cell[u], sky) : 1.0;
#pragma unroll
                for (int c = 0; c < 3; ++c) v[u][c] = map3 ? load0(map3 + (int64_t)c * plane, cell[u], sky) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (!baseline_live(cell[u], mask != nullptr, mk[u])) continue;
                double term;
                if (map3) {
                    const double sk = (v[u][0] + qu[u].x * v[u][1]) + qu[u].y * v[u][2];
                    term = wk[u] * (xk[u] - sk);
                } else {
                    term = wk[u] * xk[u];
                }
                acc = acc + term;
                hit = 1;
            }
        }
        // the fixed tree over the group's lanes (offsets that stay inside a wavefront)
        for (int off = (G < 64 ? G : 64) >> 1; off > 0; off >>= 1) {
            acc = acc + __shfl_down(acc, off, 64);
            hit |= __shfl_down(hit, off, 64);
        }
        if (G == 256) {
            const int wv = threadIdx.x >> 6;
            if ((threadIdx.x & 63) == 0) { wave_sum[wv] = acc; wave_hit[wv] = hit; }
            __syncthreads();
            if (threadIdx.x == 0) {
                acc = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
                hit = wave_hit[0] | wave_hit[1] | wave_hit[2] | wave_hit[3];
            }
            __syncthreads();                                               // before the next trip overwrites the four slots
        }
        if (lane == 0 && has && hit) out[b] = out[b] + acc;
    }
}
