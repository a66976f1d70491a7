// pxl_trip.h -- the per-lane trip loop of the streaming kernels that carry UNR points per lane ("The trip
// frame"); included by pxl_kernels.hip before pxl_elementwise.h (one translation unit, -ffp-contract=off).
//
// A block takes a contiguous chunk of blockDim.x * UNR points, a lane's points sit blockDim.x apart, and past the grid limit
// of stream_grid the first blocks go round again.  A kernel writes
//     for (Trip<UNR> trip; trip.k0 < n; trip.next()) { T v[UNR]; trip.load(p, n, v, pad); ... if (trip.k(u) < n) out[trip.k(u)] = ...; }
// Three rules keep registers and speed where the hand-written loops had them:
//   - the index products stay associated as below ((int64_t)blockIdx.x * chunk, not blockIdx.x * blockDim.x * UNR);
//   - n is the kernel's argument at every load and guard, never a copy held here;
//   - all of a trip's loads come before its first add or store.
#pragma once

template <int UNR>
struct Trip {
    int64_t chunk, k0;          // points per block and trip; the lane's first point of this trip
    __device__ __forceinline__ Trip() : chunk((int64_t)blockDim.x * UNR), k0((int64_t)blockIdx.x * chunk + threadIdx.x) {}
    __device__ __forceinline__ void next() { k0 += (int64_t)gridDim.x * chunk; }
    __device__ __forceinline__ int64_t k(int u) const { return k0 + u * blockDim.x; }
    // v[u] = p[k(u)], or pad past the end of the batch.  pad goes by value: by reference every caller took 4 more VGPRs and
    // 32 bytes of scratch
    template <class T>
    __device__ __forceinline__ void load(const T* p, int64_t n, T (&v)[UNR], T pad) const {
#pragma unroll
        for (int u = 0; u < UNR; ++u) v[u] = (k(u) < n) ? p[k(u)] : pad;
    }
};
