// pxl_kernels.hip -- gfx950 kernels + C ABI of libpixell_hip.so (see include/pixell_hip.h).
//
// Every kernel here is HBM-bound (streams or gathers of Float64) except k_toeplitz past a few taps, a stencil
// bound by the FP64 vector units whose sum order is fixed by its contract; none is GEMM-shaped, so there is
// no MFMA.  The design rules are the memory ones: 16 B per lane coalesced loads/stores, source rows
// staged through LDS once per output tile, XCD-aware tile order so neighbouring tiles share an L2.
//
// One translation unit; the kernels live in topical headers included below:
//   pxl_device.h         shared device arithmetic (Julia mod, rewind, CAR affine, sky2pix roundings, taps)
//   pxl_trip.h           the per-lane trip loop of the streaming kernels that carry several points per lane
//   pxl_elementwise.h    pix2sky / sky2pix streams            pxl_unwrap.h     unwind! scan, rewind!
//   pxl_maps.h           posmap, pixareamap                   pxl_tan.h        Gnomonic evaluators
//   pxl_reproject.h      tables, gather + register-staged     pxl_reproject_dma.h  the LDS-DMA kernel (fast path)
//                        and the tile prologue the two tile kernels share (tile_decode, tile_col, tile_direct_taps)
//   pxl_sample.h         CAR<->TAN reprojection, sampler      pxl_misc.h       FITS staging, synthetic data
//   pxl_spline.h         cubic B-spline prefilter and its transpose, order-3 reprojection, sampler and scatter-add
//   pxl_scatter.h        scatter-add, the transpose of the bilinear sampler (FP64 atomics)
//   pxl_pol.h            the polarised pointing matrix        pxl_polsolve.h   the per-pixel IQU block solve and product
//   pxl_normal.h         the normal operator y += P^T W P x of the polarised map-maker, sample and scatter fused
//   pxl_pointing.h       detector pointing expansion: boresight and detector quaternions to coordinates and responses
//   pxl_taps.h           what one sky point touches: the 2 x 2 and 4 x 4 cells, gathers, blends and adds of all point kernels
//   pxl_toeplitz.h       the banded-Toeplitz noise weight of a timestream: LDS-staged tiles, FP64 vector rate at large lambda
//   pxl_autocov.h        the gappy autocovariance of a timestream, the noise estimate behind that weight: the same tiles, lags per lane
// This file keeps the error plumbing, the host helpers the entries share (per-device state, stream-ordered scratch, table and
// workspace layouts, the front split, the unwind! ladder, `overlaps` for every aliasing rule, `tile_form` for the three launch
// forms of a reprojection plan) and the extern "C" entry points.
// The 17 pointing entries (sample, scatter, their polarised forms, the normal operator, the binned pass) go through one path:
// a PointCall says what the entry was given, check_points makes every argument check, launch_points forms the Sky2Pix and the
// grid and launches the kernel named next to its points-per-lane constant.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared   (csrc/Makefile)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <vector>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <type_traits>

#include "pxl_device.h"

using namespace pxl;

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}
#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(PXL_EHIP, "%s: %s", #expr, hipGetErrorString(e_));  \
    } while (0)

static int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(PXL_EHIP, "launch of %s failed: %s", what, hipGetErrorString(e));
    return PXL_OK;
}

static bool wcs_ok(const pxl_car_wcs* w) {
    if (!w) return false;
    for (int k = 0; k < 2; ++k)
        if (!std::isfinite(w->cdelt[k]) || !std::isfinite(w->crpix[k]) || !std::isfinite(w->crval[k]) ||
            w->cdelt[k] == 0.0)
            return false;
    return std::isfinite(w->unit) && w->unit != 0.0;
}

// full-circle test of a CAR map of nx columns: same 1e-8 threshold as enmap_geom.jl:55
static int car_periodic(const pxl_car_wcs* w, int64_t nx) {
    return fabs((double)nx * fabs(w->cdelt[0] * w->unit) - PXL_TWOPI_D) < 1e-8;
}

// Grid for 1-D streaming kernels: one contiguous chunk per block (measured best on MI355X: 69-73 % of HBM peak
// vs 57-67 % with a few thousand grid-striding blocks); grid-stride only past 2^20 blocks.
static inline unsigned stream_grid(int64_t work_items, int block) {
    int64_t nb = (work_items + block - 1) / block;
    if (nb < 1) nb = 1;
    if (nb > (1LL << 20)) nb = 1LL << 20;
    return (unsigned)nb;
}

// A launch carries blocks * threads, its work-items along x, in 32 bits: a larger grid runs blocks * threads mod 2^32 of them and
// reports no error.  An entry whose grid follows the caller's sizes therefore either refuses a grid that does not fit
// (launch_fits) or, the timestream kernels, whose grids follow n_det * n_t, launches it in chunks of PXL_CHUNK_BLOCKS blocks on the
// one stream (launch_chunks), each kernel told the number of its first block as its first argument; block0 + blockIdx.x stays
// below 2^31 (the entries' refusals).  A grid that fits one chunk is one launch.
// tests/large_tod_case.py mirrors PXL_CHUNK_BLOCKS as CHUNK_BLOCKS to size the cases that reach a second chunk: change both.
constexpr int64_t PXL_CHUNK_BLOCKS = (1 << 24) - 8;                         // 256-lane blocks; whole rounds of the 8 XCDs
static inline bool launch_fits(int64_t blocks, int threads) { return blocks <= 0xffffffffLL / threads; }
template <class Kern, class... Args>
static void launch_chunks(Kern kern, int64_t blocks, int threads, void* stream, Args... args) {
    for (int64_t b0 = 0; b0 < blocks; b0 += PXL_CHUNK_BLOCKS) {
        const int64_t nb = blocks - b0 < PXL_CHUNK_BLOCKS ? blocks - b0 : PXL_CHUNK_BLOCKS;
        hipLaunchKernelGGL(kern, dim3((unsigned)nb), dim3(threads), 0, (hipStream_t)stream, (unsigned)b0, args...);
    }
}

// do the byte ranges [a, a + a_bytes) and [b, b + b_bytes) meet?  Every aliasing rule of the library asks here; each names its own buffers.
static bool overlaps(const void* a, uintptr_t a_bytes, const void* b, uintptr_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

// A call described as named byte ranges (a null optional buffer has no bytes), and the checks such a call gets, each written once.
struct Span {
    const void* p;
    uintptr_t bytes;
    const char* name;
};
static int check_apart(const char* who, const Span& a, const Span& b) {
    if (a.bytes && b.bytes && overlaps(a.p, a.bytes, b.p, b.bytes)) return fail(PXL_EINVAL, "%s: %s overlaps %s", who, a.name, b.name);
    return PXL_OK;
}
// rd[0] is the input that wr[0] may be exactly (in place) and may not overlap otherwise.  In this order: a null buffer that has
// bytes, named (rd[0], wr[0], then the other spans read and written); 8-byte alignment of every span; the in-place pair; then
// every span written against every span read and against the spans written before it.
static int check_spans(const char* who, const Span* wr, int n_wr, const Span* rd, int n_rd) {
    auto null = [who](const Span& s) { return !s.p && s.bytes ? fail(PXL_EINVAL, "%s: null %s", who, s.name) : PXL_OK; };
    if (int rc = null(rd[0])) return rc;
    if (int rc = null(wr[0])) return rc;
    for (int k = 1; k < n_rd; ++k)
        if (int rc = null(rd[k])) return rc;
    for (int k = 1; k < n_wr; ++k)
        if (int rc = null(wr[k])) return rc;
    uintptr_t bits = 0;
    for (int k = 0; k < n_rd; ++k) bits |= (uintptr_t)rd[k].p;
    for (int k = 0; k < n_wr; ++k) bits |= (uintptr_t)wr[k].p;
    if ((bits & 7) != 0) return fail(PXL_EINVAL, "%s: buffers must be 8-byte aligned", who);
    if (wr[0].p != rd[0].p && overlaps(wr[0].p, wr[0].bytes, rd[0].p, rd[0].bytes))
        return fail(PXL_EINVAL, "%s: %s overlaps %s other than exactly (in place)", who, wr[0].name, rd[0].name);
    for (int a = 0; a < n_wr; ++a) {
        for (int k = 0; k < n_rd; ++k)
            if (!(a == 0 && k == 0))
                if (int rc = check_apart(who, wr[a], rd[k])) return rc;
        for (int k = 0; k < a; ++k)
            if (int rc = check_apart(who, wr[a], wr[k])) return rc;
    }
    return PXL_OK;
}
// the acceptance threshold of the timestream filters' fits (pxl_fit.h)
static int check_fit_rcond(const char* who, double rcond_min) {
    if (!(rcond_min >= 0.0 && rcond_min < 1.0)) return fail(PXL_EINVAL, "%s: rcond_min must lie in [0, 1) (got %g)", who, rcond_min);
    return PXL_OK;
}

static int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return (v && *v) ? atoi(v) : dflt;
}

#include "pxl_trip.h"
#include "pxl_elementwise.h"
#include "pxl_unwrap.h"
#include "pxl_maps.h"
#include "pxl_fastmath.h"
#include "pxl_tan.h"
#include "pxl_reproject.h"
#include "pxl_reproject_dma.h"
#include "pxl_taps.h"
#include "pxl_sample.h"
#include "pxl_scatter.h"
#include "pxl_misc.h"
#include "pxl_rccl.h"
#include "pxl_spread.h"
#include "pxl_distance.h"
#include "pxl_spline.h"
#include "pxl_pol.h"
#include "pxl_nearest.h"
#include "pxl_baseline.h"
#include "pxl_fit.h"
#include "pxl_polyfilter.h"
#include "pxl_modefilter.h"
#include "pxl_binfilter.h"
#include "pxl_toeplitz.h"
#include "pxl_autocov.h"
#include "pxl_normal.h"
#include "pxl_polsolve.h"
#include "pxl_pointing.h"

// ================================================================================================
// host helpers shared by the entry points
// ================================================================================================
// LDS-DMA launches (profiles/README.md): a wave's ring is halved until it fits PXL_RING_BYTES (>= 9 waves per CU), and the tile
// height is halved (down to 4 rows) while a launch has fewer than PXL_MIN_TILES tiles (3.5 per resident wave slot;
// profiles/r03_tune_mintiles*.txt)
static constexpr size_t PXL_RING_BYTES = 17 * 1024;
static constexpr int64_t PXL_MIN_TILES = 8192;

// The bilinear tables of nxo output columns and nyo output rows in one block at `mem`: [xfx nxo doubles][yfy nyo doubles]
// [xi0 nxo int32][yj0 nyo int32], 16-B aligned pieces.  mem = null: only `bytes` means anything.
struct Tables { double* xfx; double* yfy; int32_t* xi0; int32_t* yj0; size_t bytes; };
static Tables table_layout(void* mem, int64_t nxo, int64_t nyo) {
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const uintptr_t xfx = (uintptr_t)mem, yfy = xfx + up16((size_t)nxo * 8), xi0 = yfy + up16((size_t)nyo * 8),
                    yj0 = xi0 + up16((size_t)nxo * 4);
    return {(double*)xfx, (double*)yfy, (int32_t*)xi0, (int32_t*)yj0, (size_t)(yj0 + up16((size_t)nyo * 4) - xfx)};
}
// k_build_tables: division form, safe (the caller checks the launch)
static void launch_build_tables(const pxl_car_wcs& win, int64_t nx, int64_t ny, const pxl_car_wcs& wout, int64_t nxo, int64_t nyo,
                                const Tables& t, hipStream_t st) {
    hipLaunchKernelGGL(k_build_tables, dim3(stream_grid(nxo + nyo, 256)), dim3(256), 0, st, car_affine(wout),
                       sky2pix_setup(win, nx, ny, 1, PXL_FORM_DIV), nxo, nyo, t.xi0, t.xfx, t.yj0, t.yfy);
}

// LDS slots of the staging kernels by storage type: a wave access covers `cw` elements and a slot holds up to PXL_MAXCH accesses
struct SlotRule { int cw; double slack; int64_t align; };
static constexpr SlotRule kSlot64 = {128, 5.0, 2};      // + 2 (tap +1, rounding) + 1 (even alignment) + 2 slack
static constexpr SlotRule kSlot32 = {256, 8.0, 4};      // + taps, rounding and up to 3 of alignment
// footprint of the TW = cw * pairs columns of a tile at RA scale sx (source columns per output column): ceil(TW * sx) cells + slack
static int64_t seg_for(const SlotRule& r, int pairs, double sx) {
    double span = ceil((double)(r.cw * pairs) * sx) + r.slack;
    return ((int64_t)span + (r.align - 1)) & ~(r.align - 1);
}
// stageable: the slot fits, never laps the ring of pixels, and rows are not skipped wholesale (sy: source rows per output row)
static bool stageable(const SlotRule& r, int64_t sg, bool periodic, int64_t nx, double sy) {
    return (sg <= PXL_MAXCH * r.cw) && !(periodic && sg > nx) && sy <= 3.0;
}
// Launch form of a tile kernel: `pairs` accesses per lane (TW = cw * pairs columns per tile), slots of `seg` elements, and whether
// the kernel can take the map at all.  The lane width is `want`, at most `widest`, halved until the slot fits.
struct TileForm { int pairs, seg; bool ok; };
static TileForm tile_form(const SlotRule& r, int want, int widest, double sx, double sy, bool periodic, int64_t nx) {
    const int max_seg = PXL_MAXCH * r.cw;
    int pairs = std::min(want, widest);
    while (pairs > 1 && seg_for(r, pairs, sx) > max_seg) pairs >>= 1;
    const int64_t seg = seg_for(r, pairs, sx);
    return {pairs, (int)std::min<int64_t>(seg, max_seg), stageable(r, seg, periodic, nx, sy)};
}

struct pxl_reproject_plan {
    pxl_car_wcs win, wout;
    int64_t nx, ny, nc, src_row0, src_nrows;
    int64_t nxo, nyo, dst_row0, dst_nrows;
    int periodic;
    int device;
    Tables tab;        // device tables, in table_mem
    void* table_mem;
    // host copy of the row table (cells only), same arithmetic as the device
    int32_t* h_yj0;
    // launch configuration
    int variant;       // 0 auto, 1 gather, 2 staged
    TileForm dma64;    // LDS-DMA kernel, Float64 storage: lane width 1, 2 or 4 (x2 output columns per lane)
    TileForm staged64; // register-staged kernel: lane width 1 or 2.  A Float64 map takes a tile kernel only if both forms are ok
    TileForm dma32;    // LDS-DMA kernel, Float32 storage (4 elements per lane per access); ok includes nx % 4 == 0
    int dypos;
    int rh;            // tile height for Float64 maps (Float32 launches use rh32)
    int rh32;
    int dxpos;
    int ns, pf;
    int nt;            // non-temporal stores (LDS-DMA kernel, full tiles)
    double* zero_page;
    bool vec_load;
    bool tables_built;
    // sharded step: the halo exchange runs on a stream of its own, fenced by two events
    hipStream_t comm_stream;
    hipEvent_t ev_ready, ev_halo;
    int64_t cov_have_lo, cov_have_hi, cov_lo, cov_hi;     // cached pxl_reproject_plan_rows_covered answer
};

// Per-device state of the library, every access under g_dev_mu.
struct DeviceState {
    hipMemPool_t pool;            // the scratch pool below (created on first use)
    // Diagnostics of the tiled generic reprojection: how many 128 x 32 tiles of the last one-shot call took the exact path.
    // Every call counts in a counter of its own (16 bytes of its workspace, zeroed on its stream); its exact launch copies the count
    // into this per-device word, which only pxl_reproject_generic_last_tiles reads.  No call reads what another call wrote.
    unsigned int* last_exact;
    int64_t generic_tiles;        // tile count of the last one-shot call enqueued
};
static std::mutex g_dev_mu;
static DeviceState g_dev[64] = {};
// the current device's record (lock g_dev_mu before touching it); null without a current device or beyond 64 devices
static DeviceState* device_state() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    return &g_dev[dev];
}

// The scratch comes from a library-owned stream-ordered pool that keeps what it has been given: with the default
// pool (release threshold 0) every call on a drained stream went back to the driver for its memory (~250 us).
static hipMemPool_t scratch_pool() {
    DeviceState* d = device_state();
    if (!d) return nullptr;
    std::lock_guard<std::mutex> lock(g_dev_mu);
    if (!d->pool) {
        hipMemPoolProps props = {};
        props.allocType = hipMemAllocationTypePinned;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = (int)(d - g_dev);
        hipMemPool_t p = nullptr;
        if (hipMemPoolCreate(&p, &props) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        uint64_t keep = ~0ull;
        (void)hipMemPoolSetAttribute(p, hipMemPoolAttrReleaseThreshold, &keep);
        d->pool = p;
    }
    return d->pool;
}

// Scratch of one call, from the stream-ordered allocator (hipMallocAsync / hipFreeAsync): no host synchronisation.  release()
// reports a failed free; a call that returns early after alloc() frees through the destructor, on the same stream.
struct Scratch {
    char* p = nullptr;
    hipStream_t st = nullptr;
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { if (p) (void)hipFreeAsync(p, st); }
    int alloc(size_t bytes, hipStream_t stream) {
        st = stream;
        hipMemPool_t pool = scratch_pool();
        if (pool) HIP_TRY(hipMallocFromPoolAsync((void**)&p, bytes, pool, st));
        else HIP_TRY(hipMallocAsync((void**)&p, bytes, st));
        return PXL_OK;
    }
    // rc, or the free's failure as "<who>: hipFreeAsync: ..." where rc holds no error yet
    int release(const char* who, int rc) {
        hipError_t e = hipFreeAsync(p, st);
        p = nullptr;
        if (e != hipSuccess && rc == PXL_OK) rc = fail(PXL_EHIP, "%s: hipFreeAsync: %s", who, hipGetErrorString(e));
        return rc;
    }
};

// Scratch of one unwind! call.  The multi-pass fallback needs per-element scratch (5 B per value); the fused path only
// per-chunk entries.
struct UnwindWs {
    Scratch mem;
    int8_t* c; int32_t* rloc; int32_t* bsum; int32_t* boff;     // multi-pass form
    int32_t* flag;                                              // [0],[1]: multi-pass verification; [2]: fused path failed
    unsigned long long* firstnan;                               // first NaN of each coordinate row
    int2* wsum; double2* wprev;                                 // fused form: per wave chunk
    UwLink* links; unsigned int* ticket; int64_t nlinks;        // one-pass form: one link per workgroup chunk
    int64_t nb, nw;
    int U;                                                      // points per wave chunk / 64
    bool multipass;                                             // per-element scratch of the multi-pass fallback present
};

// Batches up to this size fall back (half-period ties only) to ONE gated launch of the single-block form instead
// of the ten gated launches of the multi-pass form: ~25 us less per call, where that is most of the call.  The
// single block is slower when it does run (9 us per 4096 points and pass, then the serial recurrence), so longer
// batches keep the multi-pass form, whose fixed cost no longer matters there.
static const int64_t kUnwindBlockFallbackMax = 1LL << 22;

static int unwind_ws_alloc(int64_t n, int nrow, hipStream_t st, UnwindWs* w) {
    w->nb = (n + PXL_SCAN_BLOCK - 1) / PXL_SCAN_BLOCK;
    // wave chunks of 64*U points: long enough to amortise the per-chunk work, short enough to fill the GPU
    int64_t U = n / (64 * 4096);
    U = U < 4 ? 4 : (U > 32 ? 32 : U);
    U &= ~(int64_t)(PXL_UW_G - 1);
    w->U = (int)U;
    w->nw = (n + 64 * U - 1) / (64 * U);
    if (w->nb > 0x7fffffffLL || w->nw > 0x7fffffffLL || n > 0x7fffffffLL) return fail(PXL_EINVAL, "unwind: batch too long (2^31 points)");
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    w->multipass = n > kUnwindBlockFallbackMax;
    const size_t bytes_c = w->multipass ? up((size_t)nrow * n) : 0, bytes_r = w->multipass ? up((size_t)4 * nrow * n) : 0,
                 bytes_b = w->multipass ? up((size_t)4 * nrow * w->nb) : 0;
    const size_t bytes_ws = up((size_t)w->nw * sizeof(int2)), bytes_wp = up((size_t)w->nw * sizeof(double2));
    w->nlinks = (n + PXL_UW1_CHUNK - 1) / PXL_UW1_CHUNK;
    const size_t bytes_ln = up((size_t)w->nlinks * sizeof(UwLink) + 16);
    if (int rc = w->mem.alloc(bytes_c + bytes_r + 2 * bytes_b + bytes_ws + bytes_wp + bytes_ln + 256, st)) return rc;
    char* p = w->mem.p;
    w->c = (int8_t*)p; p += bytes_c;
    w->rloc = (int32_t*)p; p += bytes_r;
    w->bsum = (int32_t*)p; p += bytes_b;
    w->boff = (int32_t*)p; p += bytes_b;
    w->wsum = (int2*)p; p += bytes_ws;
    w->wprev = (double2*)p; p += bytes_wp;
    w->links = (UwLink*)p; w->ticket = (unsigned int*)(p + (size_t)w->nlinks * sizeof(UwLink)); p += bytes_ln;
    w->flag = (int32_t*)p;
    w->firstnan = (unsigned long long*)(p + 16);
    if (hipMemsetAsync(w->flag, 0, 32, st) != hipSuccess)        // flags and the (complemented) first-NaN indices
        return fail(PXL_EHIP, "unwind: hipMemsetAsync failed");
    return PXL_OK;
}

// Fused form (pxl_unwrap.h): sums -> scan -> verify + write.  `inplace`: out aliases the input, so verify without
// storing first and store in a second launch that the device skips if the verification failed.
template <class SRC>
static int unwind_fused(const SRC& src, typename SRC::raw_t* out, int64_t n, bool inplace, UnwindWs& w, hipStream_t st) {
    const dim3 grid((unsigned)w.nw), block(64);
    int32_t* fastflag = w.flag + 2;
    hipLaunchKernelGGL((k_unwind_sums<SRC>), grid, block, 0, st, src, n, w.U, w.wsum, w.wprev, w.firstnan);
    hipLaunchKernelGGL(k_scan_wsums, dim3(1), dim3(1024), 0, st, w.nw, w.wsum);
    if (inplace) {
        hipLaunchKernelGGL((k_unwind_apply<SRC, false>), grid, block, 0, st, src, out, n, w.U, (const int2*)w.wsum,
                           (const double2*)w.wprev, (const unsigned long long*)w.firstnan, fastflag, (const int32_t*)nullptr);
        hipLaunchKernelGGL((k_unwind_apply<SRC, true>), grid, block, 0, st, src, out, n, w.U, (const int2*)w.wsum,
                           (const double2*)w.wprev, (const unsigned long long*)w.firstnan, fastflag, (const int32_t*)fastflag);
    } else {
        hipLaunchKernelGGL((k_unwind_apply<SRC, true>), grid, block, 0, st, src, out, n, w.U, (const int2*)w.wsum,
                           (const double2*)w.wprev, (const unsigned long long*)w.firstnan, fastflag, (const int32_t*)nullptr);
    }
    return check_launch("k_unwind fused");
}

// One-pass form (k_unwind_onepass: decoupled look-back; out-of-place calls only).  The links and the ticket are zeroed on the
// stream before the launch; the failure flag is the fused path's, so the same fallbacks follow.
template <class SRC>
static int unwind_onepass(const SRC& src, typename SRC::raw_t* out, int64_t n, UnwindWs& w, hipStream_t st) {
    if (w.nlinks > 0x7fffffffLL) return fail(PXL_EINVAL, "unwind: batch too long");
    hipError_t e = hipMemsetAsync(w.links, 0, (size_t)w.nlinks * sizeof(UwLink) + 16, st);
    if (e != hipSuccess) return fail(PXL_EHIP, "unwind: hipMemsetAsync: %s", hipGetErrorString(e));
    const int64_t nwg = (n + PXL_UW1_CHUNK - 1) / PXL_UW1_CHUNK;
    hipLaunchKernelGGL((k_unwind_onepass<SRC, PXL_UW1_U, PXL_UW1_UL>), dim3((unsigned)nwg), dim3(64 * PXL_UW1_WAVES), 0, st, src, out, n, w.links, w.ticket, w.flag + 2);
    return check_launch("k_unwind_onepass");
}

// Multi-pass form on a buffer that already holds m = rewind(.) - ref (see k_unwrap_* in pxl_unwrap.h).  With
// `gate` every launch is skipped on the device unless *gate != 0 (the fused form failed its verification).
static int unwind_multipass(int64_t n, int nrow, double* sky, double period, double ref, UnwindWs& w, const int32_t* gate,
                            hipStream_t st) {
    int rc = PXL_OK;
    // as a fallback these launches almost always exit at the gate: a small grid keeps that to a few microseconds each
    // (390k empty blocks cost ~85 us per launch), and the kernels grid-stride when they do run
    const unsigned cap = gate ? 2048u : 0xffffffffu;
    const unsigned g = std::min(stream_grid(n, 256), cap);
    const int64_t nb = w.nb;
    hipLaunchKernelGGL(k_unwrap_incr, dim3(g), dim3(256), 0, st, n, nrow, (const double*)sky, period, w.c, gate);
    for (int pass = 0; pass < 2 && rc == PXL_OK; ++pass) {
        const int32_t* pg = pass == 0 ? gate : w.flag;          // pass 2 runs on the device only if pass 1 flagged
        hipLaunchKernelGGL((k_scan_local<int8_t>), dim3(std::min((unsigned)nb, cap), nrow), dim3(256), 0, st, n, (const int8_t*)w.c, w.rloc, w.bsum, nb, pg);
        hipLaunchKernelGGL(k_scan_bsums, dim3(nrow), dim3(1024), 0, st, nb, (const int32_t*)w.bsum, w.boff, pg);
        hipLaunchKernelGGL(k_unwrap_verify, dim3(g), dim3(256), 0, st, n, nrow, (const double*)sky, period, w.c,
                           (const int32_t*)w.rloc, (const int32_t*)w.boff, nb, w.flag + pass, pg);
        rc = check_launch("k_unwrap scan/verify");
    }
    if (rc == PXL_OK) {
        hipLaunchKernelGGL(k_unwrap_apply, dim3(g), dim3(256), 0, st, n, nrow, sky, period, ref, (const int32_t*)w.rloc,
                           (const int32_t*)w.boff, nb, (const int32_t*)w.flag, gate);
        hipLaunchKernelGGL(k_unwind_rows, dim3(nrow), dim3(64), 0, st, n, nrow, sky, period, ref, 1, (const int32_t*)w.flag);
        rc = check_launch("k_unwrap_apply");
    }
    return rc;
}

// unwind! of n points from `src` into `out` (in place: out is the source's buffer).  Up to PXL_UWB_MAX points: one block.  Longer:
// the one-pass form (ONEPASS sources, out of place, below PXL_UW_ONEPASS_MAX: input read once, the exact rewind evaluated once) or
// the fused form (sums -> scan -> verify -> store), then, gated on the device by their failure flag, the single block, or past
// kUnwindBlockFallbackMax `pre_rewind(gate)` -- the caller's launch that leaves m = rewind(.) - ref in `out` -- and the multi-pass form.
template <bool ONEPASS, class SRC, class PRE>
static int unwind_ladder(const SRC& src, typename SRC::raw_t* out, int64_t n, bool inplace, PRE pre_rewind, hipStream_t st) {
    if (n <= PXL_UWB_MAX) {       // small batch: everything in one launch of one block
        hipLaunchKernelGGL((k_unwind_block<SRC>), dim3(1), dim3(1024), 0, st, src, out, n, (const int32_t*)nullptr);
        return check_launch("k_unwind_block");
    }
    UnwindWs w;
    int rc = unwind_ws_alloc(n, SRC::NROW, st, &w);
    if (rc) return rc;
    bool onepass = false;
    if constexpr (ONEPASS) {
        onepass = !inplace && n < PXL_UW_ONEPASS_MAX;
        if (onepass) rc = unwind_onepass(src, out, n, w, st);
    }
    if (!onepass) rc = unwind_fused(src, out, n, inplace, w, st);
    if (rc == PXL_OK) {
        const int32_t* failed = w.flag + 2;
        if (!w.multipass) {
            hipLaunchKernelGGL((k_unwind_block<SRC>), dim3(1), dim3(1024), 0, st, src, out, n, failed);
            rc = check_launch("k_unwind_block");
        } else {
            rc = pre_rewind(failed);
            if (rc == PXL_OK) rc = unwind_multipass(n, SRC::NROW, (double*)out, src.period, src.ref, w, failed, st);
        }
    }
    return w.mem.release("unwind", rc);
}

// Write-heavy kernels sweep their output in eight fronts when each front gets at least `min_per_front` of the `items`, else in
// one: `per` items per front, per * fronts grid slots.  cap > 0: a grid limit that per * fronts (rounded up to a multiple of
// `fronts`) must not pass; beyond it, one front.
struct Fronts { int fronts; int64_t per; };
static Fronts front_split(int64_t items, int min_per_front, int64_t cap) {
    int fronts = 8;
    if (items < (int64_t)min_per_front * fronts) fronts = 1;
    int64_t per = (items + fronts - 1) / fronts;
    if (cap > 0 && per * fronts > cap) { fronts = 1; per = items; }
    return {fronts, per};
}

static int check_rows(const char* who, const int64_t shape[2], int64_t row0, int64_t nrows) {
    if (!shape || shape[0] < 1 || shape[1] < 1) return fail(PXL_EINVAL, "%s: bad shape", who);
    if (row0 < 0 || nrows < 0 || row0 + nrows > shape[1])
        return fail(PXL_EINVAL, "%s: rows [%lld, %lld) outside the map (ny=%lld)", who, (long long)row0,
                    (long long)(row0 + nrows), (long long)shape[1]);
    return PXL_OK;
}

// T: the storage type, Float64 or Float32 (coordinates and weights are Float64 either way)
template <class T>
static int reproject_rows_impl(pxl_reproject_plan* pl, const T* src, T* dst, int64_t r0, int64_t nr, void* stream) {
    if (!pl) return fail(PXL_EINVAL, "execute: null plan");
    if (r0 < 0 || nr < 0 || r0 + nr > pl->dst_nrows) return fail(PXL_EINVAL, "execute: rows outside the dst window");
    if (nr == 0) return PXL_OK;
    if (!dst || (!src && pl->src_nrows > 0)) return fail(PXL_EINVAL, "execute: null src/dst");
    if (!pl->tables_built) return fail(PXL_EINVAL, "execute_rows: tables not built");
    hipStream_t st = (hipStream_t)stream;
    constexpr bool f32 = std::is_same<T, float>::value;

    ReprojParams p;
    memset(&p, 0, sizeof(p));
    p.src = src; p.dst = dst;
    p.xi0 = pl->tab.xi0; p.xfx = pl->tab.xfx; p.yj0 = pl->tab.yj0; p.yfy = pl->tab.yfy;
    p.nx = pl->nx; p.ny = pl->ny; p.src_row0 = pl->src_row0; p.src_nrows = pl->src_nrows;
    p.nxo = pl->nxo; p.dst_row0 = pl->dst_row0; p.dst_nrows = pl->dst_nrows;
    p.r0 = r0; p.nr = nr; p.nc = (int32_t)pl->nc; p.periodic = pl->periodic;

    // the kernel family, chosen once: direct gather, register-staged (Float64 maps the LDS-DMA cannot take: odd nx, unaligned
    // source, variant 2) or LDS-DMA; slot rule, launch form and tile height follow from it
    const bool aligned = (((uintptr_t)src & 15) == 0);
    const bool tiled = pl->variant != 1 && (f32 ? (pl->dma32.ok && aligned) : (pl->dma64.ok && pl->staged64.ok));
    const bool vec = f32 || (pl->vec_load && aligned);
    const bool use_dma = f32 || (vec && pl->variant != 2);
    if (!tiled) {
        int64_t work = ((pl->nxo + 1) / 2) * nr;
        dim3 g(stream_grid(work, 256), (unsigned)pl->nc);
        hipLaunchKernelGGL((k_reproject_gather<T>), g, dim3(256), 0, st, p);
        return check_launch("k_reproject_gather");
    }

    const TileForm& form = f32 ? pl->dma32 : (use_dma ? pl->dma64 : pl->staged64);
    const int cw = f32 ? kSlot32.cw : kSlot64.cw;     // elements per wave access
    int rh = f32 ? pl->rh32 : pl->rh;
    const int TW = cw * form.pairs;
    p.seg = form.seg;
    p.dxpos = pl->dxpos; p.dypos = pl->dypos;
    p.ntx = (int32_t)((pl->nxo + TW - 1) / TW);
    // tile height: the configured rh, halved while the launch would leave the chip short of waves (fewer than PXL_MIN_TILES tiles);
    // small maps and thin strips get shorter tiles
    while (rh > 4 && (int64_t)p.ntx * ((nr + rh - 1) / rh) * pl->nc < PXL_MIN_TILES) rh >>= 1;
    p.rh = rh;
    p.nty = (int32_t)((nr + rh - 1) / rh);
    p.ntiles = (int64_t)p.ntx * p.nty * pl->nc;
    p.tiles_per_xcd = (p.ntiles + 7) / 8;
    const int64_t nblocks = 8 * p.tiles_per_xcd;             // xcd_tile: one contiguous eighth of the tiles per XCD
    if (!launch_fits(nblocks, 64)) return fail(PXL_EINVAL, "execute: too many tiles (%lld)", (long long)nblocks);
    dim3 grid((unsigned)nblocks), block(64);
    if (use_dma) {
        // LDS-DMA fast path; shrink the ring if it would not fit a CU's LDS comfortably
        const size_t esz = sizeof(T);
        p.ns = pl->ns; p.pf = pl->pf; p.zero_page = pl->zero_page;
        p.nt = pl->nt != 0;
        while ((size_t)p.ns * p.seg * esz > PXL_RING_BYTES && p.ns > 4) p.ns >>= 1;
        size_t dma_lds = (size_t)p.ns * (size_t)p.seg * esz;
        const int nch = (p.seg + cw - 1) / cw;
        return launch_reproject_dma_t<T>(form.pairs, nch, grid, dma_lds, st, p);
    }
    size_t lds_bytes = (size_t)PXL_NS * (size_t)form.seg * sizeof(double);
    if (form.pairs == 2) {
        if (vec) hipLaunchKernelGGL((k_reproject_staged<2, true>), grid, block, lds_bytes, st, p);
        else     hipLaunchKernelGGL((k_reproject_staged<2, false>), grid, block, lds_bytes, st, p);
    } else {
        if (vec) hipLaunchKernelGGL((k_reproject_staged<1, true>), grid, block, lds_bytes, st, p);
        else     hipLaunchKernelGGL((k_reproject_staged<1, false>), grid, block, lds_bytes, st, p);
    }
    return check_launch("k_reproject_staged");
}

// ---- sharded step: halo rows over RCCL send/recv, interior rows while they travel, boundary rows after
template <class T>
static int sharded_step_impl(pxl_reproject_plan* pl, T* src, T* dst, int64_t own_row0, int64_t own_nrows,
                             const pxl_halo_xfer* sends, int nsends, const pxl_halo_xfer* recvs, int nrecvs,
                             void* comm, void* stream) {
    if (!pl || !src || !dst) return fail(PXL_EINVAL, "sharded_step: null plan or buffer");
    if (nsends < 0 || nrecvs < 0 || (nsends > 0 && !sends) || (nrecvs > 0 && !recvs)) return fail(PXL_EINVAL, "sharded_step: bad transfer lists");
    const int64_t lo = pl->src_row0, hi = pl->src_row0 + pl->src_nrows;
    if (own_row0 < lo || own_nrows < 0 || own_row0 + own_nrows > hi) return fail(PXL_EINVAL, "sharded_step: owned rows outside the plan's source window");
    hipStream_t st = (hipStream_t)stream;
    int rc = PXL_OK;
    const bool exchange = nsends + nrecvs > 0;
    if (exchange) {
        if (!comm) return fail(PXL_EINVAL, "sharded_step: transfers listed but no RCCL communicator");
        const RcclApi& nc = rccl_api(false);
        if (!nc.ok) return fail(PXL_ENODEV, "sharded_step: RCCL entry points not available: %s", nc.where);
        if (nc.own && !rccl_own_comm_has(comm))
            return fail(PXL_ENODEV, "sharded_step: the communicator was not created by pxl_comm_init_rank, and the only RCCL instance "
                                    "this library can see is one it loaded itself (%s): a foreign communicator belongs to another instance", nc.where);
        int nranks = 0, me = -1;
        if (nc.CommCount((ncclComm_t)comm, &nranks) != ncclSuccess || nc.CommUserRank((ncclComm_t)comm, &me) != ncclSuccess)
            return fail(PXL_EINVAL, "sharded_step: not a usable RCCL communicator");
        for (int pass = 0; pass < 2; ++pass) {
            const pxl_halo_xfer* x = pass == 0 ? sends : recvs;
            for (int i = 0; i < (pass == 0 ? nsends : nrecvs); ++i) {
                if (x[i].peer < 0 || x[i].peer >= nranks) return fail(PXL_EINVAL, "sharded_step: peer %d outside the communicator (%d ranks)", x[i].peer, nranks);
                if (x[i].nrows < 1 || x[i].row0 < lo || x[i].row0 + x[i].nrows > hi) return fail(PXL_EINVAL, "sharded_step: transfer rows outside the plan's source window");
                if (pass == 0 && (x[i].row0 < own_row0 || x[i].row0 + x[i].nrows > own_row0 + own_nrows))
                    return fail(PXL_EINVAL, "sharded_step: a rank can only send rows it owns");
            }
        }
        if (!pl->comm_stream) {
            HIP_TRY(hipStreamCreateWithFlags(&pl->comm_stream, hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&pl->ev_ready, hipEventDisableTiming));
            HIP_TRY(hipEventCreateWithFlags(&pl->ev_halo, hipEventDisableTiming));
        }
        // the exchange may start once everything queued on the caller's stream so far (the producers of src, the
        // previous step's readers of the halo rows) is done
        HIP_TRY(hipEventRecord(pl->ev_ready, st));
        HIP_TRY(hipStreamWaitEvent(pl->comm_stream, pl->ev_ready, 0));
        const size_t esz = sizeof(T);
        const ncclDataType_t dt = std::is_same<T, float>::value ? ncclFloat32 : ncclFloat64;
        ncclResult_t r = nc.GroupStart();
        // one message per component plane and transfer: rows of one plane are contiguous in the resident buffer,
        // so nothing is staged
        for (int i = 0; i < nsends && r == ncclSuccess; ++i)
            for (int64_t c = 0; c < pl->nc && r == ncclSuccess; ++c)
                r = nc.Send((const char*)src + ((c * pl->src_nrows + (sends[i].row0 - lo)) * pl->nx) * esz,
                            (size_t)(sends[i].nrows * pl->nx), dt, sends[i].peer, (ncclComm_t)comm, pl->comm_stream);
        for (int i = 0; i < nrecvs && r == ncclSuccess; ++i)
            for (int64_t c = 0; c < pl->nc && r == ncclSuccess; ++c)
                r = nc.Recv((char*)src + ((c * pl->src_nrows + (recvs[i].row0 - lo)) * pl->nx) * esz,
                            (size_t)(recvs[i].nrows * pl->nx), dt, recvs[i].peer, (ncclComm_t)comm, pl->comm_stream);
        const ncclResult_t rend = nc.GroupEnd();
        if (r == ncclSuccess) r = rend;
        if (r != ncclSuccess) return fail(PXL_EHIP, "sharded_step: RCCL send/recv failed: %s", nc.GetErrorString(r));
        HIP_TRY(hipEventRecord(pl->ev_halo, pl->comm_stream));
    }
    rc = pxl_reproject_build_tables(pl, stream);
    if (rc) return rc;
    // rows computable from the rows this rank owns run while the halo is in flight
    int64_t i_lo = 0, i_hi = pl->dst_nrows;
    if (exchange) {
        if (pl->cov_have_lo != own_row0 || pl->cov_have_hi != own_row0 + own_nrows || pl->cov_hi < pl->cov_lo) {
            rc = pxl_reproject_plan_rows_covered(pl, own_row0, own_row0 + own_nrows, &pl->cov_lo, &pl->cov_hi);
            if (rc) return rc;
            pl->cov_have_lo = own_row0; pl->cov_have_hi = own_row0 + own_nrows;
        }
        i_lo = pl->cov_lo; i_hi = pl->cov_hi;
    }
    if (i_hi > i_lo) {
        rc = reproject_rows_impl<T>(pl, src, dst, i_lo, i_hi - i_lo, stream);
        if (rc) return rc;
    }
    if (exchange) {
        HIP_TRY(hipStreamWaitEvent(st, pl->ev_halo, 0));
        if (i_hi > i_lo) {
            if (i_lo > 0) { rc = reproject_rows_impl<T>(pl, src, dst, 0, i_lo, stream); if (rc) return rc; }
            if (i_hi < pl->dst_nrows) rc = reproject_rows_impl<T>(pl, src, dst, i_hi, pl->dst_nrows - i_hi, stream);
        } else {
            rc = reproject_rows_impl<T>(pl, src, dst, 0, pl->dst_nrows, stream);
        }
    }
    return rc;
}

// the current device's word for the exact-tile count of the last one-shot generic call (DeviceState); total_tiles >= 0: record the
// tile count of the call being enqueued; total_out: the count recorded last
static unsigned int* last_exact_word(int64_t total_tiles = -1, int64_t* total_out = nullptr) {
    DeviceState* d = device_state();
    if (!d) return nullptr;
    std::lock_guard<std::mutex> lock(g_dev_mu);
    if (!d->last_exact) {
        if (hipMalloc((void**)&d->last_exact, 64) != hipSuccess || hipMemset(d->last_exact, 0, 64) != hipSuccess) {
            (void)hipGetLastError(); d->last_exact = nullptr; return nullptr;
        }
    }
    if (total_tiles >= 0) d->generic_tiles = total_tiles;
    if (total_out) *total_out = d->generic_tiles;
    return d->last_exact;
}

// geometry part of GenericParams (everything but the buffers and the component count)
static int generic_params(const char* who, const pxl_car_wcs* wcs_in, int proj_in, const int64_t* shape_in,
                          const pxl_car_wcs* wcs_out, int proj_out, const int64_t* shape_out, GenericParams* out) {
    if (!wcs_ok(wcs_in) || !wcs_ok(wcs_out)) return fail(PXL_EINVAL, "%s: invalid WCS", who);
    if (!shape_in || !shape_out) return fail(PXL_EINVAL, "%s: null shape", who);
    if (shape_in[0] < 1 || shape_in[1] < 1 || shape_out[0] < 1 || shape_out[1] < 1)
        return fail(PXL_EINVAL, "%s: shapes must be positive", who);
    if ((proj_in != PXL_PROJ_CAR && proj_in != PXL_PROJ_TAN) || (proj_out != PXL_PROJ_CAR && proj_out != PXL_PROJ_TAN))
        return fail(PXL_EINVAL, "%s: unknown projection code", who);
    GenericParams p;
    memset(&p, 0, sizeof(p));
    p.nx = shape_in[0]; p.ny = shape_in[1]; p.nc = 1;
    p.nxo = shape_out[0]; p.nyo = shape_out[1];
    p.proj_in = proj_in; p.proj_out = proj_out;
    p.periodic = (proj_in == PXL_PROJ_CAR) && car_periodic(wcs_in, p.nx);
    if (proj_out == PXL_PROJ_TAN) p.out_tan = tan_setup(*wcs_out); else p.out_car = car_affine(*wcs_out);
    if (proj_in == PXL_PROJ_TAN) p.in_tan = tan_setup(*wcs_in);
    else p.in_car = sky2pix_setup(*wcs_in, p.nx, p.ny, 1, PXL_FORM_DIV);
    *out = p;
    return PXL_OK;
}

// Workspace of the tiled generic operator at `mem`: the lattice (ntiles x 42 coordinate pairs), a flag per tile (int32) and the
// 16-byte counter of the tiles flagged for the exact path.  mem = null: only `bytes` means anything.
struct LatticeWs { double2* lat; int32_t* flag; unsigned int* counter; size_t bytes; };
static LatticeWs lattice_layout(void* mem, int64_t ntiles) {
    const size_t lat_bytes = (size_t)ntiles * (PXL_TNX * PXL_TNY) * sizeof(double2), flag_bytes = ((size_t)ntiles * 4 + 15) & ~(size_t)15;
    const uintptr_t b = (uintptr_t)mem;
    return {(double2*)b, (int32_t*)(b + lat_bytes), (unsigned int*)(b + lat_bytes + flag_bytes), lat_bytes + flag_bytes + 16};
}
// zero the counter and fill lattice and flags on the stream (p.exact_tiles is ws.counter).  Returns the memset's status; the
// caller checks the launch.
static hipError_t lattice_build(const GenericParams& p, int64_t gx, int64_t ntiles, const LatticeWs& ws, hipStream_t st) {
    hipError_t e = hipMemsetAsync(ws.counter, 0, 16, st);
    if (e == hipSuccess) hipLaunchKernelGGL(k_generic_lattice, dim3((unsigned)((ntiles + 3) / 4)), dim3(256), 0, st, p, gx, ntiles, ws.lat, ws.flag);
    return e;
}

static int spline_shape_check(const char* what, const int64_t shape[3]) {
    if (!shape) return fail(PXL_EINVAL, "%s: null shape", what);
    if (shape[0] < 4 || shape[1] < 4) return fail(PXL_EINVAL, "%s: a cubic spline needs nx, ny >= 4 (got %lld x %lld)", what, (long long)shape[0], (long long)shape[1]);
    if (shape[2] < 1 || shape[2] > 65535) return fail(PXL_EINVAL, "%s: 1 to 65535 components", what);
    if (shape[0] > 400000000 || shape[1] > 400000000) return fail(PXL_EINVAL, "%s: axis too long (<= 4e8 pixels)", what);
    return PXL_OK;
}

// the prefilter and its transpose: the same checks, scratch and pair of launches (RA, then DEC), TRANS picks the kernels
template <bool TRANS>
static int spline_prefilter_impl(const char* who, const pxl_car_wcs* wcs, const int64_t shape[3], const double* src, double* coeffs,
                                 void* stream) {
    if (!wcs_ok(wcs)) return fail(PXL_EINVAL, "%s: invalid WCS", who);
    if (int rc = spline_shape_check(who, shape)) return rc;
    if (!src || !coeffs) return fail(PXL_EINVAL, "%s: null map or output", who);
    const int64_t nx = shape[0], ny = shape[1], nc = shape[2];
    const uintptr_t bytes = (uintptr_t)nx * (uintptr_t)ny * (uintptr_t)nc * 8;
    if (overlaps(src, bytes, coeffs, bytes)) return fail(PXL_EINVAL, "%s: %s overlaps src", who, TRANS ? "dst" : "coeffs");
    const int64_t ntx = (nx + PXL_SPL_SEG - 1) / PXL_SPL_SEG, nly = (ny + PXL_SPL_LINES - 1) / PXL_SPL_LINES;
    const int64_t nty = (ny + PXL_SPL_SEG - 1) / PXL_SPL_SEG, nlx = (nx + PXL_SPL_LINES - 1) / PXL_SPL_LINES;
    if (!launch_fits(ntx * nly, 256) || !launch_fits(nty * nlx, 256)) return fail(PXL_EINVAL, "%s: map too large for one launch", who);
    hipStream_t st = (hipStream_t)stream;
    // the DEC pass reads its neighbours' warm-up rows, so the RA pass cannot leave its result where the DEC pass writes
    Scratch mem;
    if (int rc = mem.alloc(bytes, st)) return rc;
    double* rows = (double*)mem.p;
    hipLaunchKernelGGL((k_spline_prefilter<true, TRANS>), dim3((unsigned)(ntx * nly), (unsigned)nc), dim3(256), 0, st, src, rows, nx, ny,
                       car_periodic(wcs, nx), ntx);
    hipLaunchKernelGGL((k_spline_prefilter<false, TRANS>), dim3((unsigned)(nty * nlx), (unsigned)nc), dim3(256), 0, st, (const double*)rows,
                       coeffs, nx, ny, 0, nty);
    return mem.release(who, check_launch("k_spline_prefilter"));
}

template <class T>
static int build_pairs_impl(const int64_t shape_in[3], const T* src, int64_t src_nrows, T* pairs, void* stream) {
    if (pxl_sample_pairs_elems(shape_in, src_nrows) < 0) return PXL_EINVAL;
    if (!pairs || (!src && src_nrows > 0)) return fail(PXL_EINVAL, "sample_build_pairs: null buffer");
    if (((uintptr_t)pairs & 63) != 0) return fail(PXL_EINVAL, "sample_build_pairs: pair buffer must be 64-byte aligned");
    if (shape_in[0] > 0x7fffffffLL) return fail(PXL_EINVAL, "sample_build_pairs: more than 2^31 columns");
    if (shape_in[2] > 65535) return fail(PXL_EINVAL, "sample_build_pairs: more than 65535 components");
    const int64_t nx = shape_in[0], tiles = (src_nrows + 1 + PXL_POS_ROWS - 1) / PXL_POS_ROWS;
    if (tiles > 65535) return fail(PXL_EINVAL, "sample_build_pairs: more than %lld rows per call", 65535LL * PXL_POS_ROWS);
    const int64_t pitch = PairGroup<T>::groups(nx) * PairGroup<T>::E;
    const Fronts f = front_split(tiles, 16, 65535);          // grid.y limit
    dim3 grid((unsigned)((pitch + 255) / 256), (unsigned)(f.per * f.fronts), (unsigned)shape_in[2]);
    hipLaunchKernelGGL((k_build_rowpairs<T>), grid, dim3(256), 0, (hipStream_t)stream, src, nx, src_nrows, (typename Vec2T<T>::type*)pairs, f.fronts);
    return check_launch("k_build_rowpairs");
}

// ================================================================================================
// the pointing operators: sample and scatter of orders 0, 1 and 3, their polarised forms, the normal operator and the binned pass.
// An entry says what it was given (PointCall), has it checked (check_points) and names its kernel (launch_points).
// ================================================================================================
// One call.  The map is shape = (nx, ny, nc), or after rows() its rows [row0, row0 + nrows); the batch is n points at `sky`.
//   map(p)            a map the call only reads: wanted once there are points and rows
//   writes(p, planes) a map of `planes` planes (0: the map's nc) the call adds into: wanted likewise, and clear of everything read
//   reads(p, per)     `per` doubles per point (0: nc) the call reads
//   needs(p)          a buffer wanted once there are points and checked no further: a sampler's output, the row-pair copy
struct PointCall {
    struct Range { const void* p; int64_t per; };
    const char* who; const pxl_car_wcs* wcs; const int64_t* shape; int64_t n; const double* sky;
    bool window = false; int64_t row0 = 0, nrows = 0;          // nrows of a whole map: filled in by check_points
    bool cubic = false, coeffs = false, no_coeffs = false;     // order 3: the spline's shape limits; coeffs: see cubic_coeffs
    bool pol = false; const double* resp = nullptr; int mode = 0;
    bool no_map = false, no_buf = false;
    Range written[2] = {}, read[2] = {}; int nwritten = 0, nread = 0;
    bool idle = false;                                          // check_points: nothing to do, no launch

    PointCall(const char* who_, const pxl_car_wcs* wcs_, const int64_t* shape_, int64_t n_, const double* sky_)
        : who(who_), wcs(wcs_), shape(shape_), n(n_), sky(sky_) {}
    PointCall& rows(int64_t r0, int64_t nr) { window = true; row0 = r0; nrows = nr; return *this; }
    PointCall& cubic_map() { cubic = true; return *this; }
    // the order-3 samplers' coefficient array: they word a bad WCS or shape their own way and want the array even for n = 0
    PointCall& cubic_coeffs(const double* c) { cubic = coeffs = true; no_coeffs = !c; return *this; }
    // an IQU map with its 2 x n response batch; mode: 0 signal, 1 weights
    PointCall& polarised(const double* r, int m = 0) { pol = true; resp = r; mode = m; return *this; }
    PointCall& map(const void* p) { no_map |= !p; return *this; }
    PointCall& needs(const void* p) { no_buf |= !p; return *this; }
    PointCall& writes(double* p, int64_t planes) { written[nwritten++] = {p, planes}; return map(p); }
    PointCall& reads(const double* p, int64_t per) { read[nread++] = {p, per}; return needs(p); }
};

// a * b * c doubles in bytes (positive factors), or false where that passes INT64_MAX
static bool range_bytes(int64_t a, int64_t b, int64_t c, uintptr_t* bytes) {
    int64_t v;
    if (__builtin_mul_overflow(a, b, &v) || __builtin_mul_overflow(v, c, &v) || __builtin_mul_overflow(v, (int64_t)8, &v)) return false;
    *bytes = (uintptr_t)v;
    return true;
}

// Every argument check of the family, before any launch and any write: geometry, window, pointers and alignment, the cubic and the
// polarised rules, then -- once there is work -- sizes that fit and written maps clear of the points, the responses and the values.
static int check_points(PointCall& c) {
    const char* who = c.who;
    const int64_t* shape = c.shape;
    if (c.coeffs) {
        if (!wcs_ok(c.wcs)) return fail(PXL_EINVAL, "%s: invalid WCS", who);
        if (int rc = spline_shape_check(who, shape)) return rc;
    } else {
        if (!wcs_ok(c.wcs) || !shape) return fail(PXL_EINVAL, "%s: invalid WCS/shape", who);
        if (shape[0] < 1 || shape[1] < 1 || shape[2] < 1) return fail(PXL_EINVAL, "%s: shapes must be positive", who);
    }
    if (!c.window) c.nrows = shape[1];
    else if (c.row0 < 0 || c.nrows < 0 || c.row0 + c.nrows > shape[1]) return fail(PXL_EINVAL, "%s: source window outside the map", who);
    if (c.n < 0 || c.no_coeffs || (c.n > 0 && (!c.sky || c.no_buf || (c.no_map && c.nrows > 0))))
        return fail(PXL_EINVAL, "%s: null buffer or negative n", who);
    if (((uintptr_t)c.sky & 15) != 0) return fail(PXL_EINVAL, "%s: 2xN buffer must be 16-byte aligned", who);
    if (c.cubic && !c.coeffs)
        if (int rc = spline_shape_check(who, shape)) return rc;
    if (c.pol) {
        if (shape[2] != 3) return fail(PXL_EINVAL, "%s: an IQU map has exactly 3 components (got %lld)", who, (long long)shape[2]);
        if (c.mode != 0 && c.mode != 1) return fail(PXL_EINVAL, "%s: mode must be 0 (signal) or 1 (weights), not %d", who, c.mode);
        if (c.n > 0 && !c.resp) return fail(PXL_EINVAL, "%s: null response batch", who);
        if (((uintptr_t)c.resp & 15) != 0) return fail(PXL_EINVAL, "%s: 2xN response batch must be 16-byte aligned", who);
    }
    c.idle = c.n == 0 || (c.nrows == 0 && c.nwritten > 0);
    if (c.idle || c.nwritten == 0) return PXL_OK;
    uintptr_t pts = 0, rb[2] = {}, wb[2] = {};                  // bytes of a 2 x n batch, of each range read, of each map written
    bool fits = range_bytes(2, c.n, 1, &pts);
    for (int i = 0; i < c.nread; ++i) fits = fits && range_bytes(c.read[i].per ? c.read[i].per : shape[2], c.n, 1, &rb[i]);
    for (int i = 0; i < c.nwritten; ++i) fits = fits && range_bytes(c.written[i].per ? c.written[i].per : shape[2], c.nrows, shape[0], &wb[i]);
    if (!fits) return fail(PXL_EINVAL, "%s: sizes overflow", who);
    for (int i = 0; i < c.nwritten; ++i) {
        const void* dst = c.written[i].p;
        bool meets = overlaps(dst, wb[i], c.sky, pts) || (c.pol && overlaps(dst, wb[i], c.resp, pts));
        for (int k = 0; k < c.nread; ++k) meets = meets || overlaps(dst, wb[i], c.read[k].p, rb[k]);
        if (meets) return fail(PXL_EINVAL, c.pol ? "%s: dst overlaps the points, the responses or the values" : "%s: dst overlaps the points or the values", who);
    }
    return PXL_OK;
}

// The family's one launch: the map's safe, reciprocal-form Sky2Pix, blocks of 256 lanes with `per_lane` points each, then the
// kernel's own arguments as given.  A call check_points found idle launches nothing.
template <class K, class... A>
static int launch_points(const PointCall& c, const char* name, K kern, int per_lane, void* stream, A... args) {
    if (c.idle) return PXL_OK;
    const Sky2Pix s = sky2pix_setup(*c.wcs, c.shape[0], c.shape[1], 1, PXL_FORM_RECIP);
    hipLaunchKernelGGL(kern, dim3(stream_grid((c.n + per_lane - 1) / per_lane, 256)), dim3(256), 0, (hipStream_t)stream, s, args...);
    return check_launch(name);
}

template <class T>
static int sample_impl(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const T* src, int64_t src_row0,
                       int64_t src_nrows, int64_t n, const double* sky, T* out, void* stream) {
    PointCall c("sample", wcs_in, shape_in, n, sky);
    if (int rc = check_points(c.rows(src_row0, src_nrows).map(src).needs(out))) return rc;
    return launch_points(c, "k_sample_bilinear", k_sample_bilinear<T>, PXL_SUNR, stream, src, shape_in[0], shape_in[1], (int32_t)shape_in[2],
                         src_row0, src_nrows, car_periodic(wcs_in, shape_in[0]), n, (const double2*)sky, out);
}

template <class T>
static int sample_pairs_impl(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const T* pairs, int64_t src_row0,
                             int64_t src_nrows, int64_t n, const double* sky, T* out, void* stream) {
    PointCall c("sample_pairs", wcs_in, shape_in, n, sky);
    if (int rc = check_points(c.rows(src_row0, src_nrows).needs(pairs).needs(out))) return rc;
    if (((uintptr_t)pairs & 63) != 0) return fail(PXL_EINVAL, "sample_pairs: pair buffer must be 64-byte aligned");
    if (shape_in[0] > 0x7fffffffLL) return fail(PXL_EINVAL, "sample_pairs: more than 2^31 columns");
    return launch_points(c, "k_sample_pairs", k_sample_pairs<T>, PairsUnroll<T>::value, stream, (const typename Vec2T<T>::type*)pairs,
                         shape_in[0], shape_in[1], (int32_t)shape_in[2], src_row0, src_nrows, car_periodic(wcs_in, shape_in[0]), n,
                         (const double2*)sky, out);
}

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

int pxl_version(void) { return PXL_VERSION; }

size_t pxl_last_error(char* buf, size_t n) {
    size_t len = strlen(g_err);
    if (buf && n) {
        size_t m = len < n - 1 ? len : n - 1;
        memcpy(buf, g_err, m);
        buf[m] = 0;
    }
    return len;
}

int pxl_release_scratch(void) {
    DeviceState* d = device_state();
    if (!d) return fail(PXL_ENODEV, "release_scratch: no current device");
    std::lock_guard<std::mutex> lock(g_dev_mu);
    if (d->pool && hipMemPoolTrimTo(d->pool, 0) != hipSuccess) return fail(PXL_EHIP, "release_scratch: hipMemPoolTrimTo failed");
    return PXL_OK;
}

// ---- placement probe (pxl_spread.h): eight store fronts, four in each of two windows
int pxl_mem_probe_pair(void* a, void* b, size_t window_bytes, int reps, float* us, void* stream) {
    if (!a || !b || !us) return fail(PXL_EINVAL, "mem_probe_pair: null argument");
    if (window_bytes < (64u << 20) || (window_bytes & 63) != 0 || (((uintptr_t)a | (uintptr_t)b) & 15) != 0)
        return fail(PXL_EINVAL, "mem_probe_pair: windows of at least 64 MiB, a multiple of 64 bytes, 16-byte aligned");
    if (reps < 1 || reps > 99) return fail(PXL_EINVAL, "mem_probe_pair: 1..99 repetitions");
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    {
        hipError_t ec = hipEventCreate(&e1);
        if (ec != hipSuccess) { (void)hipEventDestroy(e0); return fail(PXL_EHIP, "hipEventCreate(&e1): %s", hipGetErrorString(ec)); }
    }
    std::vector<float> t(reps);
    int rc = PXL_OK;
    for (int r = -1; r < reps && rc == PXL_OK; ++r) {
        hipError_t e = hipEventRecord(e0, st);
        hipLaunchKernelGGL(k_spread_probe, dim3(8 * 256 * 2), dim3(256), 0, st, (char*)a, (char*)b, window_bytes / 4);
        if (e == hipSuccess) e = hipGetLastError();          // a refused launch would otherwise time an empty interval
        if (e == hipSuccess) e = hipEventRecord(e1, st);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e != hipSuccess) rc = fail(PXL_EHIP, "mem_probe_pair: %s", hipGetErrorString(e));
        else if (r >= 0) t[r] = ms * 1000.f;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    std::sort(t.begin(), t.end());
    *us = t[reps / 2];
    return PXL_OK;
}

#include "pxl_place.h"

int pxl_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(PXL_ENODEV, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

int pxl_pix2sky_car_f64(const pxl_car_wcs* wcs, int64_t n, const double* pix, double* sky, int wrap_mode,
                        void* stream) {
    if (!wcs_ok(wcs)) return fail(PXL_EINVAL, "pix2sky: invalid WCS");
    if (n < 0 || (n > 0 && (!pix || !sky))) return fail(PXL_EINVAL, "pix2sky: null buffer or negative n");
    if (wrap_mode < PXL_WRAP_NONE || wrap_mode > PXL_WRAP_UNWIND) return fail(PXL_EINVAL, "pix2sky: bad wrap_mode %d", wrap_mode);
    if ((((uintptr_t)pix | (uintptr_t)sky) & 15) != 0) return fail(PXL_EINVAL, "pix2sky: 2xN buffers must be 16-byte aligned");
    if (n == 0) return PXL_OK;
    hipStream_t st = (hipStream_t)stream;
    CarAffine c = car_affine(*wcs);
    const int mode = wrap_mode == PXL_WRAP_REWIND ? 1 : (wrap_mode == PXL_WRAP_UNWIND ? 2 : 0);
    if (wrap_mode == PXL_WRAP_NONE) {          // affine only: one point per lane per trip
        hipLaunchKernelGGL((k_pix2sky_pairs<1>), dim3(stream_grid(n, 256)), dim3(256), 0, st, c, n, (const double2*)pix,
                           (double2*)sky, mode, (const int32_t*)nullptr);
        return check_launch("k_pix2sky_pairs");
    }
    const dim3 pgrid(stream_grid((n + 1) / 2, 256));
    if (wrap_mode != PXL_WRAP_UNWIND) {
        hipLaunchKernelGGL((k_pix2sky_pairs<2>), pgrid, dim3(256), 0, st, c, n, (const double2*)pix, (double2*)sky, mode,
                           (const int32_t*)nullptr);
        return check_launch("k_pix2sky_pairs");
    }
    // in-place (pix == sky) is fine, a partial overlap is not: every unwind form reads inputs other waves / rounds
    // have not consumed yet while it stores (checked before ANY launch, the single-block form included)
    const uintptr_t bytes = (uintptr_t)n * 16;
    if (pix != sky && overlaps(pix, bytes, sky, bytes)) return fail(PXL_EINVAL, "pix2sky: pix and sky may alias exactly or not at all");
    // safe=true: one block, or on a long batch the one-pass / fused rewind + verified scan and the fallbacks only if its check fails
    auto pre_rewind = [&](const int32_t* gate) {
        hipLaunchKernelGGL((k_pix2sky_pairs<2>), dim3(std::min(pgrid.x, 2048u)), dim3(256), 0, st, c, n, (const double2*)pix, (double2*)sky, 2, gate);
        return check_launch("k_pix2sky_pairs");
    };
    return unwind_ladder<true>(UwSrcPix2{c, (const double2*)pix, PXL_TWOPI_D, 0.0, 1.0 / PXL_TWOPI_D}, (double2*)sky, n, pix == sky, pre_rewind, st);
}

int pxl_rewind_f64(double* a, int64_t n, double period, double ref_angle, void* stream) {
    if (n < 0 || (n > 0 && !a)) return fail(PXL_EINVAL, "rewind: null buffer or negative n");
    if (!(period > 0.0) || !std::isfinite(period) || !std::isfinite(ref_angle)) return fail(PXL_EINVAL, "rewind: period must be positive and finite");
    if (n == 0) return PXL_OK;
    hipLaunchKernelGGL(k_rewind, dim3(stream_grid((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, n, a, period, ref_angle, 0,
                       (const int32_t*)nullptr);
    return check_launch("k_rewind");
}

int pxl_unwind_f64(double* a, int64_t n, int nrow, double period, double ref_angle, void* stream) {
    if (n < 0 || (n > 0 && !a)) return fail(PXL_EINVAL, "unwind: null buffer or negative n");
    if (nrow != 1 && nrow != 2) return fail(PXL_EINVAL, "unwind: nrow must be 1 (vector) or 2 (2xN batch)");
    if (!(period > 0.0) || !std::isfinite(period) || !std::isfinite(ref_angle)) return fail(PXL_EINVAL, "unwind: period must be positive and finite");
    if (nrow == 2 && ((uintptr_t)a & 15) != 0) return fail(PXL_EINVAL, "unwind: 2xN buffer must be 16-byte aligned");
    if (n == 0) return PXL_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 rgrid(stream_grid(((int64_t)nrow * n + 3) / 4, 256));
    auto pre_rewind = [&](const int32_t* gate) {
        hipLaunchKernelGGL(k_rewind, dim3(std::min(rgrid.x, 2048u)), dim3(256), 0, st, (int64_t)nrow * n, a, period, ref_angle, 1, gate);
        return check_launch("k_rewind");
    };
    if (nrow == 2) return unwind_ladder<false>(UwSrcAng2{(const double2*)a, period, ref_angle, 1.0 / period}, (double2*)a, n, true, pre_rewind, st);
    return unwind_ladder<false>(UwSrcAng1{(const double*)a, period, ref_angle, 1.0 / period}, a, n, true, pre_rewind, st);
}

int pxl_pix2sky_car_soa_f64(const pxl_car_wcs* wcs, int64_t n, const double* ipix, const double* jpix,
                            double* ra, double* dec, int safe, void* stream) {
    if (!wcs_ok(wcs)) return fail(PXL_EINVAL, "pix2sky_soa: invalid WCS");
    if (n < 0 || (n > 0 && (!ipix || !jpix || !ra || !dec))) return fail(PXL_EINVAL, "pix2sky_soa: null buffer or negative n");
    if (n == 0) return PXL_OK;
    const int vec = ((((uintptr_t)ipix | (uintptr_t)jpix | (uintptr_t)ra | (uintptr_t)dec) & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(k_pix2sky_soa, dim3(stream_grid((n + 1) / 2, 256)), dim3(256), 0, (hipStream_t)stream,
                       car_affine(*wcs), n, ipix, jpix, ra, dec, safe ? 1 : 0, vec);
    return check_launch("k_pix2sky_soa");
}

int pxl_sky2pix_car_f64(const pxl_car_wcs* wcs, const int64_t shape[2], int64_t n, const double* sky,
                        double* pix, int safe, int form, void* stream) {
    if (!wcs_ok(wcs) || !shape) return fail(PXL_EINVAL, "sky2pix: invalid WCS/shape");
    if (n < 0 || (n > 0 && (!pix || !sky))) return fail(PXL_EINVAL, "sky2pix: null buffer or negative n");
    if (form < 0 || form > 2) return fail(PXL_EINVAL, "sky2pix: bad form %d", form);
    if ((((uintptr_t)pix | (uintptr_t)sky) & 15) != 0) return fail(PXL_EINVAL, "sky2pix: 2xN buffers must be 16-byte aligned");
    if (n == 0) return PXL_OK;
    Sky2Pix s = sky2pix_setup(*wcs, shape[0], shape[1], safe ? 1 : 0, form);
    if (safe)
        hipLaunchKernelGGL((k_sky2pix_pairs<2>), dim3(stream_grid((n + 1) / 2, 256)), dim3(256), 0,
                           (hipStream_t)stream, s, n, (const double2*)sky, (double2*)pix);
    else
        hipLaunchKernelGGL((k_sky2pix_pairs<1>), dim3(stream_grid(n, 256)), dim3(256), 0,
                           (hipStream_t)stream, s, n, (const double2*)sky, (double2*)pix);
    return check_launch("k_sky2pix_pairs");
}

int pxl_sky2pix_car_soa_f64(const pxl_car_wcs* wcs, const int64_t shape[2], int64_t n, const double* ra,
                            const double* dec, double* ipix, double* jpix, int safe, int form, void* stream) {
    if (!wcs_ok(wcs) || !shape) return fail(PXL_EINVAL, "sky2pix_soa: invalid WCS/shape");
    if (n < 0 || (n > 0 && (!ipix || !jpix || !ra || !dec))) return fail(PXL_EINVAL, "sky2pix_soa: null buffer or negative n");
    if (form < 0 || form > 2) return fail(PXL_EINVAL, "sky2pix_soa: bad form %d", form);
    if (n == 0) return PXL_OK;
    Sky2Pix s = sky2pix_setup(*wcs, shape[0], shape[1], safe ? 1 : 0, form);
    const int vec = ((((uintptr_t)ipix | (uintptr_t)jpix | (uintptr_t)ra | (uintptr_t)dec) & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(k_sky2pix_soa, dim3(stream_grid((n + 1) / 2, 256)), dim3(256), 0, (hipStream_t)stream, s, n, ra,
                       dec, ipix, jpix, vec);
    return check_launch("k_sky2pix_soa");
}

int pxl_posmap_car_f64(const pxl_car_wcs* wcs, const int64_t shape[2], int64_t row0, int64_t nrows,
                       double* ra, double* dec, int safe, void* stream) {
    if (!wcs_ok(wcs)) return fail(PXL_EINVAL, "posmap: invalid WCS");
    int rc = check_rows("posmap", shape, row0, nrows);
    if (rc) return rc;
    if (nrows == 0) return PXL_OK;
    if (!ra || !dec) return fail(PXL_EINVAL, "posmap: null output");
    if (nrows > 65535LL * PXL_POS_ROWS) return fail(PXL_EINVAL, "posmap: more than %lld rows per call", 65535LL * PXL_POS_ROWS);
    const int64_t nych = (nrows + PXL_POS_ROWS - 1) / PXL_POS_ROWS;
    const Fronts f = front_split(nych, 16, 65535);           // grid.y limit
    dim3 grid((unsigned)(((shape[0] + 1) / 2 + 255) / 256), (unsigned)(f.per * f.fronts));
    hipLaunchKernelGGL(k_posmap_car, grid, dim3(256), 0, (hipStream_t)stream,
                       car_affine(*wcs), shape[0], row0, nrows, ra, dec, safe ? 1 : 0, f.fronts);
    return check_launch("k_posmap_car");
}

int pxl_pixareamap_car_f64(const pxl_car_wcs* wcs, const int64_t shape[2], int64_t row0, int64_t nrows,
                           double* area, void* stream) {
    if (!wcs_ok(wcs)) return fail(PXL_EINVAL, "pixareamap: invalid WCS");
    int rc = check_rows("pixareamap", shape, row0, nrows);
    if (rc) return rc;
    if (nrows == 0) return PXL_OK;
    if (!area) return fail(PXL_EINVAL, "pixareamap: null output");
    if ((shape[0] & 1) == 0 && ((uintptr_t)area & 15) == 0) {
        // one contiguous chunk of the map per block (pairs of pixels, 16-byte stores)
        const int64_t total = shape[0] / 2 * nrows;
        const int64_t nchunks = (total + PXL_AREA_CHUNK - 1) / PXL_AREA_CHUNK;
        const Fronts f = front_split(nchunks, 64, 0);
        hipLaunchKernelGGL(k_pixareamap_chunks, dim3((unsigned)(f.per * f.fronts)), dim3(256), 0,
                           (hipStream_t)stream, car_affine(*wcs), shape[0], row0, nrows, area, f.fronts);
        return check_launch("k_pixareamap_chunks");
    }
    // odd nx / unaligned map: one row per blockIdx.y (<= 65535 per launch)
    for (int64_t r = 0; r < nrows; r += 65535) {
        int64_t nr = (nrows - r < 65535) ? nrows - r : 65535;
        unsigned gx = (unsigned)std::max<int64_t>(1, ((shape[0] + 1) / 2 + 2047) / 2048);   // ~8 pairs per lane
        hipLaunchKernelGGL(k_pixareamap_car, dim3(gx, (unsigned)nr), dim3(256), 0, (hipStream_t)stream,
                           car_affine(*wcs), shape[0], row0 + r, nr, area + r * shape[0]);
        int rc2 = check_launch("k_pixareamap_car");
        if (rc2) return rc2;
    }
    return PXL_OK;
}

int pxl_distance_transform_car_f64(const pxl_car_wcs* wcs, const int64_t shape[2], const double* m, double* dist,
                                   void* stream) {
    if (!wcs_ok(wcs)) return fail(PXL_EINVAL, "distance_transform: invalid WCS");
    if (!shape || shape[0] < 1 || shape[1] < 1) return fail(PXL_EINVAL, "distance_transform: shape must be positive");
    if (!m || !dist) return fail(PXL_EINVAL, "distance_transform: null map or output");
    const int64_t nx = shape[0], ny = shape[1];
    if (nx > PXL_SDT_MAX_NX) return fail(PXL_EINVAL, "distance_transform: rows of more than %d pixels", PXL_SDT_MAX_NX);
    if (ny > 0x7fffffffLL) return fail(PXL_EINVAL, "distance_transform: more than 2^31 - 1 rows");
    const uintptr_t bytes = (uintptr_t)nx * (uintptr_t)ny * 8;
    if (overlaps(m, bytes, dist, bytes)) return fail(PXL_EINVAL, "distance_transform: dist overlaps m");
    const CarAffine c = car_affine(*wcs);
    // the left/right candidates of a row cover the circle once
    if ((double)nx * fabs(c.da) > PXL_TWOPI_D + 1e-8) return fail(PXL_EINVAL, "distance_transform: the map spans more than 360 degrees of RA");
    // the column choice needs cos(DEC) >= 0 on every row, and the sweep needs DEC monotone along the rows.  Full-sky CC pole
    // rows sit exactly on +-Float64(pi/2), where cos > 0; a row e (<= 1e-9) beyond a pole is accepted, at up to 4e more in d^2
    const bool up = c.dd > 0.0;
    double prev = 0.0;
    for (int64_t j = 1; j <= ny; ++j) {
        const double d = rewind(p2s_dec(c, (double)j), PXL_TWOPI_D, 0.0);
        if (!(fabs(d) <= PXL_PI_D / 2 + 1e-9))
            return fail(PXL_EINVAL, "distance_transform: row %lld lies beyond a pole (DEC %.17g rad)", (long long)j, d);
        if (j > 1 && (up ? d < prev : d > prev)) return fail(PXL_EINVAL, "distance_transform: DEC is not monotone along the rows");
        prev = d;
    }
    // scratch from the library's stream-ordered pool: RA and DEC tables, the best column per pixel (int32), the chains (int64)
    auto up256 = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t npix = (size_t)nx * (size_t)ny;
    const size_t b_csa = up256((size_t)nx * 16), b_csd = up256((size_t)ny * 16), b_best = up256(npix * 4), b_chain = npix * 8;
    hipStream_t st = (hipStream_t)stream;
    Scratch mem;
    if (int rc = mem.alloc(b_csa + b_csd + b_best + b_chain, st)) return rc;
    char* ws = mem.p;
    double2* csa = (double2*)ws;
    double2* csd = (double2*)(ws + b_csa);
    int32_t* best = (int32_t*)(ws + b_csa + b_csd);
    long long* chain = (long long*)(ws + b_csa + b_csd + b_best);
    hipLaunchKernelGGL(k_sdt_tables, dim3(stream_grid(nx + ny, 256)), dim3(256), 0, st, c, nx, ny, csa, csd);
    const size_t lds = (size_t)((nx + 63) / 64) * 16;
    hipLaunchKernelGGL(k_sdt_rows, dim3((unsigned)ny), dim3(PXL_SDT_ROW_THREADS), lds, st, m, nx, (const double2*)csa, best);
    hipLaunchKernelGGL(k_sdt_columns, dim3((unsigned)((nx + 63) / 64)), dim3(64), 0, st, (const int32_t*)best, nx, ny, up ? 1 : 0,
                       (const double2*)csa, (const double2*)csd, chain, dist);
    return mem.release("distance_transform", check_launch("k_sdt_rows / k_sdt_columns"));
}

int pxl_sky2pix_tan_f64(const pxl_car_wcs* wcs, int64_t n, const double* ra, const double* dec, double* ipix,
                        double* jpix, void* stream) {
    if (!wcs_ok(wcs)) return fail(PXL_EINVAL, "sky2pix_tan: invalid WCS");
    if (n < 0 || (n > 0 && (!ipix || !jpix || !ra || !dec))) return fail(PXL_EINVAL, "sky2pix_tan: null buffer or negative n");
    if (n == 0) return PXL_OK;
    const bool vec = ((((uintptr_t)ra | (uintptr_t)dec | (uintptr_t)ipix | (uintptr_t)jpix) & 15) == 0);
    const dim3 grid(stream_grid((n + 1) / 2, 256));
    if (vec) hipLaunchKernelGGL((k_tan_points<true, false>), grid, dim3(256), 0, (hipStream_t)stream, tan_setup(*wcs), n, ra, dec, ipix, jpix);
    else     hipLaunchKernelGGL((k_tan_points<false, false>), grid, dim3(256), 0, (hipStream_t)stream, tan_setup(*wcs), n, ra, dec, ipix, jpix);
    return check_launch("k_tan_points (sky2pix)");
}

int pxl_pix2sky_tan_f64(const pxl_car_wcs* wcs, int64_t n, const double* ipix, const double* jpix, double* ra,
                        double* dec, void* stream) {
    if (!wcs_ok(wcs)) return fail(PXL_EINVAL, "pix2sky_tan: invalid WCS");
    if (n < 0 || (n > 0 && (!ipix || !jpix || !ra || !dec))) return fail(PXL_EINVAL, "pix2sky_tan: null buffer or negative n");
    if (n == 0) return PXL_OK;
    const bool vec = ((((uintptr_t)ra | (uintptr_t)dec | (uintptr_t)ipix | (uintptr_t)jpix) & 15) == 0);
    const dim3 grid(stream_grid((n + 1) / 2, 256));
    if (vec) hipLaunchKernelGGL((k_tan_points<true, true>), grid, dim3(256), 0, (hipStream_t)stream, tan_setup(*wcs), n, ipix, jpix, ra, dec);
    else     hipLaunchKernelGGL((k_tan_points<false, true>), grid, dim3(256), 0, (hipStream_t)stream, tan_setup(*wcs), n, ipix, jpix, ra, dec);
    return check_launch("k_tan_points (pix2sky)");
}

int pxl_posmap_tan_f64(const pxl_car_wcs* wcs, const int64_t shape[2], int64_t row0, int64_t nrows, double* ra,
                       double* dec, void* stream) {
    if (!wcs_ok(wcs)) return fail(PXL_EINVAL, "posmap_tan: invalid WCS");
    int rc = check_rows("posmap_tan", shape, row0, nrows);
    if (rc) return rc;
    if (nrows == 0) return PXL_OK;
    if (!ra || !dec) return fail(PXL_EINVAL, "posmap_tan: null output");
    const int64_t nchunk = (shape[0] + 511) / 512;                 // 512 RA pixels per block
    const int64_t nrb = (nrows + PXL_TAN_ROWS - 1) / PXL_TAN_ROWS;   // PXL_TAN_ROWS rows per block
    if (!launch_fits(nchunk * nrb, 256)) return fail(PXL_EINVAL, "posmap_tan: map too large for one launch");
    const bool vec = (shape[0] % 2 == 0) && ((((uintptr_t)ra | (uintptr_t)dec) & 15) == 0);
    // maps of at least one tile: the grid form (anchors + closed-form differences + interpolation, pxl_tan.h); a small map or a
    // patch where the grid does not pay: the per-pixel evaluation
    // The grid form pays when a 128-column tile spans at most ~2 degrees (pixels up to ~1 arcmin: beyond that the degree-8 interpolant
    // misses its 2^-55 rad check and the rows fall back to the per-pixel path after paying for the lattice) and the patch centre is
    // not next to a pole (there most rows fail the small-angle preconditions)
    const TanParams tp0 = tan_setup(*wcs);
    const bool grid_pays = fabs(tp0.uos) * PXL_TG_W <= 0.04 && fabs(tp0.cd0) >= 0.3;
    if (grid_pays && shape[0] >= PXL_TG_W && nrows >= 8) {
        const int64_t ntx = (shape[0] + PXL_TG_W - 1) / PXL_TG_W, nty = (nrows + PXL_TG_ROWS - 1) / PXL_TG_ROWS;
        const Fronts f = front_split(nty, 4, 0);
        const int64_t nbx = (ntx + 3) / 4, nblk = f.per * f.fronts * nbx;
        if (launch_fits(nblk, 256)) {
            if (vec) hipLaunchKernelGGL((k_posmap_tan_grid<true>), dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, tp0, shape[0], row0, nrows, ntx, f.per, f.fronts, ra, dec);
            else     hipLaunchKernelGGL((k_posmap_tan_grid<false>), dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, tp0, shape[0], row0, nrows, ntx, f.per, f.fronts, ra, dec);
            return check_launch("k_posmap_tan_grid");
        }
    }
    const dim3 grid((unsigned)(nchunk * nrb));
    if (vec) hipLaunchKernelGGL((k_posmap_tan<true>), grid, dim3(256), 0, (hipStream_t)stream, tan_setup(*wcs), shape[0], row0, nrows, nchunk, ra, dec);
    else     hipLaunchKernelGGL((k_posmap_tan<false>), grid, dim3(256), 0, (hipStream_t)stream, tan_setup(*wcs), shape[0], row0, nrows, nchunk, ra, dec);
    return check_launch("k_posmap_tan");
}

// ---- reprojection plan -------------------------------------------------------------------------

int pxl_reproject_plan_create(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], int64_t src_row0,
                              int64_t src_nrows, const pxl_car_wcs* wcs_out, const int64_t shape_out[2],
                              int64_t dst_row0, int64_t dst_nrows, pxl_reproject_plan** out) {
    if (!out) return fail(PXL_EINVAL, "plan_create: null plan pointer");
    *out = nullptr;
    if (!wcs_ok(wcs_in) || !wcs_ok(wcs_out)) return fail(PXL_EINVAL, "plan_create: invalid WCS");
    if (!shape_in || !shape_out) return fail(PXL_EINVAL, "plan_create: null shape");
    if (shape_in[0] < 1 || shape_in[1] < 1 || shape_in[2] < 1 || shape_out[0] < 1 || shape_out[1] < 1)
        return fail(PXL_EINVAL, "plan_create: shapes must be positive");
    // int32 cell tables and 32-bit byte offsets within a source row: nx * 8 must stay below 2^32
    if (shape_in[0] > 400000000 || shape_in[1] > 1000000000 || shape_out[0] > 1000000000 || shape_out[1] > 1000000000)
        return fail(PXL_EINVAL, "plan_create: axis too long (source RA axis <= 4e8, others <= 1e9 pixels)");
    if (src_row0 < 0 || src_nrows < 0 || src_row0 + src_nrows > shape_in[1])
        return fail(PXL_EINVAL, "plan_create: source window outside the map");
    if (dst_row0 < 0 || dst_nrows < 0 || dst_row0 + dst_nrows > shape_out[1])
        return fail(PXL_EINVAL, "plan_create: destination window outside the map");

    pxl_reproject_plan* pl = new (std::nothrow) pxl_reproject_plan();     // value-initialised: all members zero
    if (!pl) return fail(PXL_ENOMEM, "plan_create: host allocation failed");
    pl->cov_lo = 0; pl->cov_hi = -1;                                        // no cached interior yet
    pl->win = *wcs_in; pl->wout = *wcs_out;
    pl->nx = shape_in[0]; pl->ny = shape_in[1]; pl->nc = shape_in[2];
    pl->src_row0 = src_row0; pl->src_nrows = src_nrows;
    pl->nxo = shape_out[0]; pl->nyo = shape_out[1];
    pl->dst_row0 = dst_row0; pl->dst_nrows = dst_nrows;
    pl->periodic = car_periodic(wcs_in, pl->nx);
    pl->tables_built = false;

    hipError_t e = hipGetDevice(&pl->device);
    if (e != hipSuccess) { delete pl; return fail(PXL_ENODEV, "hipGetDevice: %s", hipGetErrorString(e)); }

    // the tables, and behind them the plan's own zero page
    const size_t nyo = (size_t)pl->nyo, off_zero = table_layout(nullptr, pl->nxo, pl->nyo).bytes, total = off_zero + 64;
    e = hipMalloc(&pl->table_mem, total);
    if (e != hipSuccess) { delete pl; return fail(PXL_ENOMEM, "plan_create: hipMalloc(%zu): %s", total, hipGetErrorString(e)); }
    char* base = (char*)pl->table_mem;
    e = hipMemset(base + off_zero, 0, 64);
    if (e != hipSuccess) { (void)hipFree(pl->table_mem); delete pl; return fail(PXL_EHIP, "plan_create: hipMemset: %s", hipGetErrorString(e)); }
    pl->zero_page = (double*)(base + off_zero);
    pl->tab = table_layout(base, pl->nxo, pl->nyo);

    // host copy of the row cells (identical arithmetic: fmod/div/floor are exact or correctly rounded)
    pl->h_yj0 = new (std::nothrow) int32_t[nyo];
    if (!pl->h_yj0) { (void)hipFree(pl->table_mem); delete pl; return fail(PXL_ENOMEM, "plan_create: host allocation failed"); }
    CarAffine co = car_affine(pl->wout);
    Sky2Pix si = sky2pix_setup(pl->win, pl->nx, pl->ny, 1, PXL_FORM_DIV);
    for (int64_t j = 0; j < pl->nyo; ++j) {
        double fr;
        split_cell(s2p_y(si, p2s_dec(co, (double)(j + 1))), &pl->h_yj0[j], &fr);
    }

    // ---- choose the launch configuration from the RA scale (source columns per output column)
    double sx = fabs((pl->wout.cdelt[0] * pl->wout.unit) / (pl->win.cdelt[0] * pl->win.unit));
    pl->dxpos = ((pl->wout.cdelt[0] * pl->wout.unit) / (pl->win.cdelt[0] * pl->win.unit)) > 0 ? 1 : 0;
    pl->dypos = ((pl->wout.cdelt[1] * pl->wout.unit) / (pl->win.cdelt[1] * pl->win.unit)) > 0 ? 1 : 0;
    double sy = fabs((pl->wout.cdelt[1] * pl->wout.unit) / (pl->win.cdelt[1] * pl->win.unit));
    // Defaults, one line each (the measurements behind them: docs/DESIGN_history_r04.md):
    // tile height: 4 rows coarsening 2x, 16 from equal resolution to 2x refinement, 8 at 4x (profiles/r03_tune_other3_*.txt, r04_tune_nt_bursts.txt)
    pl->rh = env_int("PXL_REPROJECT_RH", sy >= 1.5 ? 4 : (sy > 0.3 ? 16 : 8));
    if (pl->rh < 1) pl->rh = 1;
    if (pl->rh > 64) pl->rh = 64;          // one lane per tile row holds the row-table entry
    pl->rh32 = env_int("PXL_REPROJECT_RH", 32);      // Float32 maps (4 pixels per lane) prefer 32 in both regimes
    if (pl->rh32 < 1) pl->rh32 = 1;
    if (pl->rh32 > 64) pl->rh32 = 64;
    // ring depth: 8 slots, 4 (twice the resident waves) when the source fits the Infinity Cache (profiles/r03_tune_pf2_cfg2.txt)
    pl->ns = env_int("PXL_REPROJECT_NS", (double)pl->nx * (double)pl->ny * (double)pl->nc * 8.0 <= 128.0 * 1048576.0 ? 4 : 8);
    if (pl->ns < 4) pl->ns = 4;
    while (pl->ns & (pl->ns - 1)) pl->ns &= pl->ns - 1;       // power of two
    if (pl->ns > 64) pl->ns = 64;
    // prefetch distance in OUTPUT rows: as many SOURCE rows ahead as the ring has free slots (profiles/r03_tune_pf_cfg3.txt)
    {
        int want_pf = (int)ceil((pl->ns - 2) / (sy > 0.125 ? sy : 0.125));
        pl->pf = env_int("PXL_REPROJECT_PF", want_pf < 3 ? 3 : want_pf);
    }
    // non-temporal stores keep the column tables in the L2 and win on every launch timed in bursts (profiles/r04_tune_nt_bursts.txt)
    pl->nt = env_int("PXL_REPROJECT_NT", 1);
    if (pl->pf < 0) pl->pf = 0;
    // lane width: 2 pairs (256 columns per wave) at equal resolution; up-sampling in RA takes 512 columns per wave
    // (4 KB contiguous per store row, half the column-halo re-reads): +15 % at >= ~3x (10800 -> 43200) and, since the
    // row loop keeps one interpolant per source row in registers, +2 % at 2x (round 3: 1.794 vs 1.830 ms on the
    // 1' -> 0.5' map in a slow placement, 1.631 vs 1.638 ms in a fast one; profiles/r03_tune_cfg3_a.txt)
    int want = env_int("PXL_REPROJECT_PAIRS", sx <= 0.55 ? 4 : 2);
    if (want != 1 && want != 2 && want != 4) want = 2;
    // Float32 storage (a wave access covers 256 elements, slots hold up to 5 x 256): 4 pixels per lane make up-sampling VALU-heavy,
    // narrower tiles there (measured 0.98 vs 1.18 ms)
    int want32 = env_int("PXL_REPROJECT_PAIRS", sx < 0.75 ? 1 : 2);
    if (want32 != 1 && want32 != 2 && want32 != 4) want32 = 2;
    pl->dma64 = tile_form(kSlot64, want, 4, sx, sy, pl->periodic, pl->nx);
    pl->staged64 = tile_form(kSlot64, want, 2, sx, sy, pl->periodic, pl->nx);
    pl->dma32 = tile_form(kSlot32, want32, 4, sx, sy, pl->periodic, pl->nx);
    pl->dma32.ok = pl->dma32.ok && (pl->nx % 4 == 0);
    pl->vec_load = (pl->nx % 2 == 0);
    *out = pl;
    return PXL_OK;
}

int pxl_reproject_plan_set_variant(pxl_reproject_plan* pl, int variant) {
    if (!pl || variant < 0 || variant > 2) return fail(PXL_EINVAL, "set_variant: bad argument");
    pl->variant = variant;
    return PXL_OK;
}

int pxl_reproject_plan_destroy(pxl_reproject_plan* pl) {
    if (!pl) return PXL_OK;
    if (pl->comm_stream) {
        (void)hipStreamSynchronize(pl->comm_stream);
        (void)hipEventDestroy(pl->ev_ready);
        (void)hipEventDestroy(pl->ev_halo);
        (void)hipStreamDestroy(pl->comm_stream);
    }
    if (pl->table_mem) (void)hipFree(pl->table_mem);
    delete[] pl->h_yj0;
    delete pl;
    return PXL_OK;
}

int pxl_reproject_build_tables(pxl_reproject_plan* pl, void* stream) {
    if (!pl) return fail(PXL_EINVAL, "build_tables: null plan");
    launch_build_tables(pl->win, pl->nx, pl->ny, pl->wout, pl->nxo, pl->nyo, pl->tab, (hipStream_t)stream);
    int rc = check_launch("k_build_tables");
    if (rc == PXL_OK) pl->tables_built = true;
    return rc;
}

int pxl_reproject_execute_rows(pxl_reproject_plan* pl, const double* src, double* dst, int64_t r0, int64_t nr,
                               void* stream) {
    return reproject_rows_impl(pl, src, dst, r0, nr, stream);
}

int pxl_reproject_execute_rows_f32(pxl_reproject_plan* pl, const float* src, float* dst, int64_t r0, int64_t nr,
                                   void* stream) {
    return reproject_rows_impl(pl, src, dst, r0, nr, stream);
}

int pxl_reproject_execute(pxl_reproject_plan* pl, const double* src, double* dst, void* stream) {
    int rc = pxl_reproject_build_tables(pl, stream);
    if (rc) return rc;
    return pxl_reproject_execute_rows(pl, src, dst, 0, pl->dst_nrows, stream);
}

int pxl_reproject_execute_f32(pxl_reproject_plan* pl, const float* src, float* dst, void* stream) {
    int rc = pxl_reproject_build_tables(pl, stream);
    if (rc) return rc;
    return pxl_reproject_execute_rows_f32(pl, src, dst, 0, pl->dst_nrows, stream);
}

int pxl_reproject_plan_src_rows(const pxl_reproject_plan* pl, int64_t* lo, int64_t* hi) {
    if (!pl || !lo || !hi) return fail(PXL_EINVAL, "plan_src_rows: null argument");
    int64_t l = INT64_MAX, h = INT64_MIN;
    for (int64_t r = 0; r < pl->dst_nrows; ++r) {
        int64_t j0 = pl->h_yj0[pl->dst_row0 + r];
        for (int64_t j = j0; j <= j0 + 1; ++j)
            if (j >= 1 && j <= pl->ny) { if (j - 1 < l) l = j - 1; if (j > h) h = j; }
    }
    if (l > h) { l = 0; h = 0; }
    *lo = l; *hi = h;
    return PXL_OK;
}

int pxl_reproject_plan_rows_covered(const pxl_reproject_plan* pl, int64_t have_lo, int64_t have_hi, int64_t* lo,
                                    int64_t* hi) {
    if (!pl || !lo || !hi) return fail(PXL_EINVAL, "plan_rows_covered: null argument");
    // longest run of output rows (relative) whose in-map taps j0, j0+1 all lie in [have_lo, have_hi)
    int64_t best_lo = 0, best_hi = 0, cur_lo = -1;
    for (int64_t r = 0; r <= pl->dst_nrows; ++r) {
        bool ok = false;
        if (r < pl->dst_nrows) {
            int64_t j0 = pl->h_yj0[pl->dst_row0 + r];
            ok = true;
            for (int64_t j = j0; j <= j0 + 1; ++j)
                if (j >= 1 && j <= pl->ny && !(j - 1 >= have_lo && j - 1 < have_hi)) ok = false;
        }
        if (ok) { if (cur_lo < 0) cur_lo = r; }
        else if (cur_lo >= 0) {
            if (r - cur_lo > best_hi - best_lo) { best_lo = cur_lo; best_hi = r; }
            cur_lo = -1;
        }
    }
    *lo = best_lo; *hi = best_hi;
    return PXL_OK;
}

// ---- communicator helpers for hosts without an RCCL binding of their own (Julia, C): thin wrappers over
// ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy, resolved through pxl_rccl.h
int pxl_comm_unique_id(void* id128) {
    if (!id128) return fail(PXL_EINVAL, "comm_unique_id: null buffer (PXL_COMM_ID_BYTES bytes)");
    const RcclApi& nc = rccl_api(true);
    if (!nc.ok) return fail(PXL_ENODEV, "comm_unique_id: RCCL not available: %s", nc.where);
    static_assert(sizeof(ncclUniqueId) == PXL_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId id;
    ncclResult_t r = nc.GetUniqueId(&id);
    if (r != ncclSuccess) return fail(PXL_EHIP, "comm_unique_id: ncclGetUniqueId: %s", nc.GetErrorString(r));
    memcpy(id128, &id, sizeof id);
    return PXL_OK;
}

int pxl_comm_init_rank(const void* id128, int rank, int nranks, void** comm) {
    if (!id128 || !comm) return fail(PXL_EINVAL, "comm_init_rank: null argument");
    *comm = nullptr;
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(PXL_EINVAL, "comm_init_rank: rank %d outside [0, %d)", rank, nranks);
    const RcclApi& nc = rccl_api(true);
    if (!nc.ok) return fail(PXL_ENODEV, "comm_init_rank: RCCL not available: %s", nc.where);
    ncclUniqueId id;
    memcpy(&id, id128, sizeof id);
    ncclComm_t c = nullptr;
    ncclResult_t r = nc.CommInitRank(&c, nranks, id, rank);          // collective over the nranks callers; uses the current device
    if (r != ncclSuccess) return fail(PXL_EHIP, "comm_init_rank: ncclCommInitRank: %s", nc.GetErrorString(r));
    rccl_own_comm_add((void*)c);
    *comm = (void*)c;
    return PXL_OK;
}

int pxl_comm_destroy(void* comm) {
    if (!comm) return PXL_OK;
    if (!rccl_own_comm_erase(comm)) return fail(PXL_EINVAL, "comm_destroy: not a communicator created by pxl_comm_init_rank");
    const RcclApi& nc = rccl_api(false);
    if (!nc.ok) return fail(PXL_ENODEV, "comm_destroy: RCCL not available: %s", nc.where);
    ncclResult_t r = nc.CommDestroy((ncclComm_t)comm);
    if (r != ncclSuccess) return fail(PXL_EHIP, "comm_destroy: ncclCommDestroy: %s", nc.GetErrorString(r));
    return PXL_OK;
}

const char* pxl_comm_backend(void) {
    // a diagnostic: it probes for an instance already in the process but latches nothing (pxl_rccl.h); the text lives in
    // a thread-local buffer, valid until this thread asks again
    static thread_local char where[256];
    const RcclApi nc = rccl_api(false);
    snprintf(where, sizeof where, "%s", nc.where);
    return where;
}

int pxl_reproject_sharded_step_f64(pxl_reproject_plan* plan, double* src, double* dst, int64_t own_row0, int64_t own_nrows,
                                   const pxl_halo_xfer* sends, int nsends, const pxl_halo_xfer* recvs, int nrecvs,
                                   void* rccl_comm, void* stream) {
    return sharded_step_impl(plan, src, dst, own_row0, own_nrows, sends, nsends, recvs, nrecvs, rccl_comm, stream);
}

int pxl_reproject_sharded_step_f32(pxl_reproject_plan* plan, float* src, float* dst, int64_t own_row0, int64_t own_nrows,
                                   const pxl_halo_xfer* sends, int nsends, const pxl_halo_xfer* recvs, int nrecvs,
                                   void* rccl_comm, void* stream) {
    return sharded_step_impl(plan, src, dst, own_row0, own_nrows, sends, nsends, recvs, nrecvs, rccl_comm, stream);
}

int pxl_reproject_car_bilinear_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* src,
                                   const pxl_car_wcs* wcs_out, const int64_t shape_out[2], double* dst,
                                   void* stream) {
    if (!shape_in || !shape_out) return fail(PXL_EINVAL, "reproject: null shape");
    pxl_reproject_plan* pl = nullptr;
    int rc = pxl_reproject_plan_create(wcs_in, shape_in, 0, shape_in[1], wcs_out, shape_out, 0, shape_out[1], &pl);
    if (rc) return rc;
    rc = pxl_reproject_execute(pl, src, dst, stream);
    if (rc == PXL_OK) {
        hipError_t e = hipStreamSynchronize((hipStream_t)stream);
        if (e != hipSuccess) rc = fail(PXL_EHIP, "reproject: %s", hipGetErrorString(e));
    }
    pxl_reproject_plan_destroy(pl);
    return rc;
}

int pxl_reproject_generic_last_tiles(int64_t* exact_tiles, int64_t* total_tiles, void* stream) {
    if (!exact_tiles || !total_tiles) return fail(PXL_EINVAL, "generic_last_tiles: null argument");
    int64_t total = 0;
    unsigned int* c = last_exact_word(-1, &total);
    if (!c) return fail(PXL_ENODEV, "generic_last_tiles: no counter on this device");
    unsigned int v = 0;
    HIP_TRY(hipMemcpyAsync(&v, c, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    *exact_tiles = v; *total_tiles = total;
    return PXL_OK;
}

// ---- the generic operator with its lattice kept (include/pixell_hip.h)
struct pxl_generic_plan {
    GenericParams p;             // geometry; src / dst / nc are filled per execute
    int64_t gx, gy, ntiles, exact;
    char* mem;
    LatticeWs ws;                // in mem
    int device;
};

int pxl_generic_plan_create(const pxl_car_wcs* wcs_in, int proj_in, const int64_t shape_in[2],
                            const pxl_car_wcs* wcs_out, int proj_out, const int64_t shape_out[2],
                            void* stream, pxl_generic_plan** plan) {
    if (!plan) return fail(PXL_EINVAL, "generic_plan_create: null result");
    *plan = nullptr;
    GenericParams p;
    int rc = generic_params("generic_plan_create", wcs_in, proj_in, shape_in, wcs_out, proj_out, shape_out, &p);
    if (rc) return rc;
    const int64_t gx = (p.nxo + PXL_TW - 1) / PXL_TW, gy = (p.nyo + PXL_TH - 1) / PXL_TH;
    if (gy > 65535) return fail(PXL_EINVAL, "generic_plan_create: more than 65 535 tile rows (use the one-shot entry)");
    const int64_t ntiles = gx * gy;
    pxl_generic_plan* pl = new (std::nothrow) pxl_generic_plan();
    if (!pl) return fail(PXL_ENOMEM, "generic_plan_create: out of host memory");
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipGetDevice(&pl->device);
    if (e == hipSuccess) e = hipMalloc((void**)&pl->mem, lattice_layout(nullptr, ntiles).bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); delete pl; return fail(PXL_EHIP, "generic_plan_create: %s", hipGetErrorString(e)); }
    pl->ws = lattice_layout(pl->mem, ntiles);
    pl->gx = gx; pl->gy = gy; pl->ntiles = ntiles;
    p.exact_tiles = pl->ws.counter; p.exact_tiles_last = nullptr;
    pl->p = p;
    unsigned int host_count = 0;
    e = lattice_build(p, gx, ntiles, pl->ws, st);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&host_count, pl->ws.counter, 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipFree(pl->mem); delete pl; return fail(PXL_EHIP, "generic_plan_create: %s", hipGetErrorString(e)); }
    pl->exact = host_count;
    *plan = pl;
    return PXL_OK;
}

int pxl_generic_plan_execute(const pxl_generic_plan* plan, int64_t ncomp, const double* src, double* dst, void* stream) {
    if (!plan) return fail(PXL_EINVAL, "generic_plan_execute: null plan");
    if (ncomp < 1 || ncomp > 0x7fffffff) return fail(PXL_EINVAL, "generic_plan_execute: component count must be positive");
    if (!src || !dst) return fail(PXL_EINVAL, "generic_plan_execute: null src/dst");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != plan->device) return fail(PXL_EINVAL, "generic_plan_execute: plan belongs to device %d, current device is %d", plan->device, dev);
    GenericParams p = plan->p;
    p.src = src; p.dst = dst; p.nc = (int32_t)ncomp;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_reproject_generic_tiled3, dim3((unsigned)plan->gx, (unsigned)plan->gy), dim3(256), 0, st, p, (const double2*)plan->ws.lat, (const int32_t*)plan->ws.flag);
    if (plan->exact > 0)       // known on the host since the plan was made: no launch at all for the usual patch
        hipLaunchKernelGGL(k_reproject_generic_exact_tiles, dim3((unsigned)std::min<int64_t>(plan->ntiles, 256)), dim3(256), 0, st, p, (const int32_t*)plan->ws.flag, plan->gx, plan->ntiles);
    return check_launch("k_reproject_generic_tiled3 (plan)");
}

int pxl_generic_plan_tiles(const pxl_generic_plan* plan, int64_t* exact_tiles, int64_t* total_tiles) {
    if (!plan || !exact_tiles || !total_tiles) return fail(PXL_EINVAL, "generic_plan_tiles: null argument");
    *exact_tiles = plan->exact; *total_tiles = plan->ntiles;
    return PXL_OK;
}

int pxl_generic_plan_destroy(pxl_generic_plan* plan) {
    if (!plan) return PXL_OK;
    hipError_t e = plan->mem ? hipFree(plan->mem) : hipSuccess;
    delete plan;
    if (e != hipSuccess) return fail(PXL_EHIP, "generic_plan_destroy: %s", hipGetErrorString(e));
    return PXL_OK;
}

int pxl_reproject_generic_bilinear_f64(const pxl_car_wcs* wcs_in, int proj_in, const int64_t shape_in[3],
                                       const double* src, const pxl_car_wcs* wcs_out, int proj_out,
                                       const int64_t shape_out[2], double* dst, void* stream) {
    GenericParams p;
    int rcp = generic_params("reproject_generic", wcs_in, proj_in, shape_in, wcs_out, proj_out, shape_out, &p);
    if (rcp) return rcp;
    if (shape_in[2] < 1) return fail(PXL_EINVAL, "reproject_generic: shapes must be positive");
    if (!src || !dst) return fail(PXL_EINVAL, "reproject_generic: null src/dst");
    p.src = src; p.dst = dst; p.nc = (int32_t)shape_in[2];
    // PXL_GENERIC_EXACT=1: per-pixel evaluation of the coordinates (the definition; cross-check and fallback of the
    // tiled kernel, which interpolates them per 128 x 32 tile within PXL_TILED_TOL pixel)
    const int64_t gx = (p.nxo + PXL_TW - 1) / PXL_TW, gy = (p.nyo + PXL_TH - 1) / PXL_TH;
    if (env_int("PXL_GENERIC_EXACT", 0) || gy > 65535) {
        hipLaunchKernelGGL(k_reproject_generic, dim3(stream_grid(p.nxo * p.nyo, 256)), dim3(256), 0, (hipStream_t)stream, p);
        return check_launch("k_reproject_generic");
    }
    // per-tile lattice (42 coordinate pairs) + flag + this call's count of exact tiles, from the library's stream-ordered scratch pool
    const int64_t ntiles = gx * gy;
    p.exact_tiles_last = last_exact_word(ntiles);
    hipStream_t st = (hipStream_t)stream;
    Scratch mem;
    if (int rc = mem.alloc(lattice_layout(nullptr, ntiles).bytes, st)) return rc;
    const LatticeWs ws = lattice_layout(mem.p, ntiles);
    p.exact_tiles = ws.counter;
    hipError_t me = lattice_build(p, gx, ntiles, ws, st);
    if (me != hipSuccess) {
        (void)hipGetLastError();
        return fail(PXL_EHIP, "reproject_generic: hipMemsetAsync: %s", hipGetErrorString(me));
    }
    hipLaunchKernelGGL(k_reproject_generic_tiled3, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, st, p, (const double2*)ws.lat, (const int32_t*)ws.flag);
    hipLaunchKernelGGL(k_reproject_generic_exact_tiles, dim3((unsigned)std::min<int64_t>(ntiles, 256)), dim3(256), 0, st, p, (const int32_t*)ws.flag, gx, ntiles);
    return mem.release("reproject_generic", check_launch("k_reproject_generic_tiled3"));
}

int pxl_sample_car_bilinear_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* src,
                                int64_t src_row0, int64_t src_nrows, int64_t n, const double* sky, double* out,
                                void* stream) {
    return sample_impl(wcs_in, shape_in, src, src_row0, src_nrows, n, sky, out, stream);
}

// the transpose of pxl_sample_car_bilinear_f64: the same geometry, every check before any write
int pxl_scatter_car_bilinear_f64(const pxl_car_wcs* wcs, const int64_t shape[3], double* dst, int64_t row0, int64_t nrows,
                                 int64_t n, const double* sky, const double* vals, void* stream) {
    PointCall c("scatter", wcs, shape, n, sky);
    if (int rc = check_points(c.rows(row0, nrows).reads(vals, 0).writes(dst, 0))) return rc;
    return launch_points(c, "k_scatter_bilinear", k_scatter_bilinear, PXL_SUNR, stream, dst, shape[0], shape[1], (int32_t)shape[2], row0, nrows,
                         car_periodic(wcs, shape[0]), n, (const double2*)sky, vals);
}

int pxl_sample_car_bilinear_f32(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const float* src,
                                int64_t src_row0, int64_t src_nrows, int64_t n, const double* sky, float* out,
                                void* stream) {
    return sample_impl(wcs_in, shape_in, src, src_row0, src_nrows, n, sky, out, stream);
}

// ---- cubic B-spline interpolation (pxl_spline.h) ----------------------------------------------------------
int pxl_spline_prefilter_car_f64(const pxl_car_wcs* wcs, const int64_t shape[3], const double* src, double* coeffs, void* stream) {
    return spline_prefilter_impl<false>("spline_prefilter", wcs, shape, src, coeffs, stream);
}

int pxl_spline_prefilter_transpose_car_f64(const pxl_car_wcs* wcs, const int64_t shape[3], const double* src, double* dst, void* stream) {
    return spline_prefilter_impl<true>("spline_prefilter_transpose", wcs, shape, src, dst, stream);
}

int pxl_reproject_car_cubic_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* coeffs,
                                const pxl_car_wcs* wcs_out, const int64_t shape_out[2], double* dst, void* stream) {
    if (!wcs_ok(wcs_in) || !wcs_ok(wcs_out)) return fail(PXL_EINVAL, "reproject_cubic: invalid WCS");
    if (int rc = spline_shape_check("reproject_cubic", shape_in)) return rc;
    if (!shape_out || shape_out[0] < 1 || shape_out[1] < 1) return fail(PXL_EINVAL, "reproject_cubic: output shape must be positive");
    if (shape_out[0] > 1000000000 || shape_out[1] > 65535LL * PXL_SPL_TH) return fail(PXL_EINVAL, "reproject_cubic: output axis too long");
    if (!coeffs || !dst) return fail(PXL_EINVAL, "reproject_cubic: null coefficients or output");
    const int64_t nx = shape_in[0], ny = shape_in[1], nc = shape_in[2], nxo = shape_out[0], nyo = shape_out[1];
    const uintptr_t cb = (uintptr_t)nx * (uintptr_t)ny * (uintptr_t)nc * 8, db = (uintptr_t)nxo * (uintptr_t)nyo * (uintptr_t)nc * 8;
    if (overlaps(coeffs, cb, dst, db)) return fail(PXL_EINVAL, "reproject_cubic: dst overlaps coeffs");
    hipStream_t st = (hipStream_t)stream;
    // the bilinear plan's tables, in scratch
    Scratch mem;
    if (int rc = mem.alloc(table_layout(nullptr, nxo, nyo).bytes, st)) return rc;
    const Tables t = table_layout(mem.p, nxo, nyo);
    SplineReproj p;
    p.coeffs = coeffs; p.dst = dst;
    p.xfx = t.xfx; p.yfy = t.yfy; p.xi0 = t.xi0; p.yj0 = t.yj0;
    p.nx = nx; p.ny = ny; p.nxo = nxo; p.nyo = nyo; p.periodic = car_periodic(wcs_in, nx);
    launch_build_tables(*wcs_in, nx, ny, *wcs_out, nxo, nyo, t, st);
    hipLaunchKernelGGL(k_reproject_cubic, dim3((unsigned)((nxo + 255) / 256), (unsigned)((nyo + PXL_SPL_TH - 1) / PXL_SPL_TH), (unsigned)nc),
                       dim3(256), 0, st, p);
    return mem.release("reproject_cubic", check_launch("k_reproject_cubic"));
}

int pxl_sample_car_cubic_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* coeffs, int64_t n,
                             const double* sky, double* out, void* stream) {
    PointCall c("sample_cubic", wcs_in, shape_in, n, sky);
    if (int rc = check_points(c.cubic_coeffs(coeffs).needs(out))) return rc;
    return launch_points(c, "k_sample_cubic", k_sample_cubic, 1, stream, coeffs, shape_in[0], shape_in[1], (int32_t)shape_in[2],
                         car_periodic(wcs_in, shape_in[0]), n, (const double2*)sky, out);
}

// the transpose of pxl_sample_car_cubic_f64's evaluation: the sampler's geometry, every check before any write
int pxl_scatter_car_cubic_f64(const pxl_car_wcs* wcs, const int64_t shape[3], double* dst, int64_t n, const double* sky,
                              const double* vals, void* stream) {
    PointCall c("scatter_cubic", wcs, shape, n, sky);
    if (int rc = check_points(c.cubic_map().reads(vals, 0).writes(dst, 0))) return rc;
    return launch_points(c, "k_scatter_cubic", k_scatter_cubic, PXL_CUNR, stream, dst, shape[0], shape[1], (int32_t)shape[2],
                         car_periodic(wcs, shape[0]), n, (const double2*)sky, vals);
}

// ---- the polarised pointing matrix (pxl_pol.h): polarised() adds the IQU map, the response batch and the mode
int pxl_sample_car_pol_bilinear_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* src, int64_t src_row0,
                                    int64_t src_nrows, int64_t n, const double* sky, const double* resp, double* out, void* stream) {
    PointCall c("sample_pol", wcs_in, shape_in, n, sky);
    if (int rc = check_points(c.rows(src_row0, src_nrows).polarised(resp).map(src).needs(out))) return rc;
    return launch_points(c, "k_sample_pol_bilinear", k_sample_pol_bilinear, PXL_PSUNR, stream, src, shape_in[0], shape_in[1], src_row0, src_nrows,
                         car_periodic(wcs_in, shape_in[0]), n, (const double2*)sky, (const double2*)resp, out);
}

int pxl_sample_car_pol_cubic_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* coeffs, int64_t n,
                                 const double* sky, const double* resp, double* out, void* stream) {
    PointCall c("sample_pol_cubic", wcs_in, shape_in, n, sky);
    if (int rc = check_points(c.cubic_coeffs(coeffs).polarised(resp).needs(out))) return rc;
    return launch_points(c, "k_sample_pol_cubic", k_sample_pol_cubic, 1, stream, coeffs, shape_in[0], shape_in[1],
                         car_periodic(wcs_in, shape_in[0]), n, (const double2*)sky, (const double2*)resp, out);
}

int pxl_scatter_car_pol_bilinear_f64(const pxl_car_wcs* wcs, const int64_t shape[3], double* dst, int64_t row0, int64_t nrows, int64_t n,
                                     const double* sky, const double* resp, const double* vals, int mode, void* stream) {
    PointCall c("scatter_pol", wcs, shape, n, sky);
    if (int rc = check_points(c.rows(row0, nrows).polarised(resp, mode).reads(vals, 1).writes(dst, mode ? 6 : 3))) return rc;
    return launch_points(c, "k_scatter_pol_bilinear", mode ? k_scatter_pol_bilinear<6> : k_scatter_pol_bilinear<3>, PXL_SUNR, stream, dst,
                         shape[0], shape[1], row0, nrows, car_periodic(wcs, shape[0]), n, (const double2*)sky, (const double2*)resp, vals);
}

int pxl_scatter_car_pol_cubic_f64(const pxl_car_wcs* wcs, const int64_t shape[3], double* dst, int64_t n, const double* sky,
                                  const double* resp, const double* vals, int mode, void* stream) {
    PointCall c("scatter_pol_cubic", wcs, shape, n, sky);
    if (int rc = check_points(c.cubic_map().polarised(resp, mode).reads(vals, 1).writes(dst, mode ? 6 : 3))) return rc;
    return launch_points(c, "k_scatter_pol_cubic", mode ? k_scatter_pol_cubic<6> : k_scatter_pol_cubic<3>, PXL_CUNR, stream, dst, shape[0],
                         shape[1], car_periodic(wcs, shape[0]), n, (const double2*)sky, (const double2*)resp, vals);
}

// ---- the normal operator y += P^T W P x (pxl_normal.h): the sampler's checks on x, the scatter's on y with w in
// the place of the values, and x itself one more range y may not meet
int pxl_normal_car_pol_bilinear_f64(const pxl_car_wcs* wcs, const int64_t shape[3], const double* x3, double* y3, int64_t n,
                                    const double* sky, const double* resp, const double* w, void* stream) {
    PointCall c("normal_pol", wcs, shape, n, sky);
    if (int rc = check_points(c.polarised(resp).map(x3).reads(w, 1).writes(y3, 3))) return rc;
    const uintptr_t mb = c.idle ? 0 : (uintptr_t)(3 * shape[1] * shape[0]) * 8;
    if (overlaps(y3, mb, x3, mb)) return fail(PXL_EINVAL, "normal_pol: y overlaps x");
    return launch_points(c, "k_normal_pol_bilinear", k_normal_pol_bilinear, PXL_NUNR, stream, x3, y3, shape[0], shape[1],
                         car_periodic(wcs, shape[0]), n, (const double2*)sky, (const double2*)resp, w);
}

// ---- nearest-pixel (order 0) pointing (pxl_nearest.h): each entry makes its bilinear counterpart's checks and
// builds the same Sky2Pix, so the positions are the order-1 positions bit for bit
int pxl_sample_car_nearest_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* src, int64_t src_row0,
                               int64_t src_nrows, int64_t n, const double* sky, double* out, void* stream) {
    PointCall c("sample_nearest", wcs_in, shape_in, n, sky);
    if (int rc = check_points(c.rows(src_row0, src_nrows).map(src).needs(out))) return rc;
    return launch_points(c, "k_sample_nearest", k_sample_nearest, PXL_ZUNR, stream, src, shape_in[0], shape_in[1], (int32_t)shape_in[2], src_row0,
                         src_nrows, car_periodic(wcs_in, shape_in[0]), n, (const double2*)sky, out);
}

int pxl_scatter_car_nearest_f64(const pxl_car_wcs* wcs, const int64_t shape[3], double* dst, int64_t row0, int64_t nrows,
                                int64_t n, const double* sky, const double* vals, void* stream) {
    PointCall c("scatter_nearest", wcs, shape, n, sky);
    if (int rc = check_points(c.rows(row0, nrows).reads(vals, 0).writes(dst, 0))) return rc;
    return launch_points(c, "k_scatter_nearest", k_scatter_nearest, PXL_ZUNR, stream, dst, shape[0], shape[1], (int32_t)shape[2], row0, nrows,
                         car_periodic(wcs, shape[0]), n, (const double2*)sky, vals);
}

int pxl_sample_car_pol_nearest_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* src, int64_t src_row0,
                                   int64_t src_nrows, int64_t n, const double* sky, const double* resp, double* out, void* stream) {
    PointCall c("sample_pol_nearest", wcs_in, shape_in, n, sky);
    if (int rc = check_points(c.rows(src_row0, src_nrows).polarised(resp).map(src).needs(out))) return rc;
    return launch_points(c, "k_sample_pol_nearest", k_sample_pol_nearest, PXL_ZUNR, stream, src, shape_in[0], shape_in[1], src_row0, src_nrows,
                         car_periodic(wcs_in, shape_in[0]), n, (const double2*)sky, (const double2*)resp, out);
}

int pxl_scatter_car_pol_nearest_f64(const pxl_car_wcs* wcs, const int64_t shape[3], double* dst, int64_t row0, int64_t nrows, int64_t n,
                                    const double* sky, const double* resp, const double* vals, int mode, void* stream) {
    PointCall c("scatter_pol_nearest", wcs, shape, n, sky);
    if (int rc = check_points(c.rows(row0, nrows).polarised(resp, mode).reads(vals, 1).writes(dst, mode ? 6 : 3))) return rc;
    return launch_points(c, "k_scatter_pol_nearest", mode ? k_scatter_pol_nearest<6> : k_scatter_pol_nearest<3>, PXL_ZUNR, stream, dst,
                         shape[0], shape[1], row0, nrows, car_periodic(wcs, shape[0]), n, (const double2*)sky, (const double2*)resp, vals);
}

// the fused pass: the samples d and their weights w read, the two maps written, each clear of everything read and of the other
int pxl_bin_car_pol_nearest_f64(const pxl_car_wcs* wcs, const int64_t shape[3], double* rhs3, double* weights6, int64_t n,
                                const double* sky, const double* resp, const double* d, const double* w, void* stream) {
    PointCall c("bin_pol_nearest", wcs, shape, n, sky);
    if (int rc = check_points(c.polarised(resp).reads(d, 1).reads(w, 1).writes(rhs3, 3).writes(weights6, 6))) return rc;
    const uintptr_t pb = c.idle ? 0 : (uintptr_t)(shape[1] * shape[0]) * 8;
    if (overlaps(rhs3, 3 * pb, weights6, 6 * pb)) return fail(PXL_EINVAL, "bin_pol_nearest: rhs3 overlaps weights6");
    return launch_points(c, "k_bin_pol_nearest", k_bin_pol_nearest, PXL_ZUNR, stream, rhs3, weights6, shape[0], shape[1],
                         car_periodic(wcs, shape[0]), n, (const double2*)sky, (const double2*)resp, d, w);
}

// ---- the two passes of the destriper (pxl_baseline.h).  What both entries check beyond check_points: the chunk's
// layout, that there is a d or an a, and the sizes n = n_det * n_chunk and nb = n_det * n_base.  `small`: every sample index,
// time and the baseline length fit 31 bits, so the kernels divide in 32.
struct BaselineCall { int64_t n = 0, nb = 0, b_lo = 0, nseg = 0; int small = 0; };
static int check_baselines(const char* who, int64_t n_det, int64_t n_chunk, int64_t t0, int64_t len, int64_t n_base, const double* d,
                           const double* a, BaselineCall* bc) {
    if (n_det < 0 || n_chunk < 0 || t0 < 0 || n_base < 0)
        return fail(PXL_EINVAL, "%s: n_det, n_chunk, t0 and n_base may not be negative (got %lld, %lld, %lld, %lld)", who,
                    (long long)n_det, (long long)n_chunk, (long long)t0, (long long)n_base);
    if (len < 1) return fail(PXL_EINVAL, "%s: baseline_len must be at least 1 (got %lld)", who, (long long)len);
    int64_t t1, v;
    if (__builtin_add_overflow(t0, n_chunk, &t1)) return fail(PXL_EINVAL, "%s: t0 + n_chunk overflows", who);
    if (n_chunk > 0 && (t1 - 1) / len >= n_base)
        return fail(PXL_EINVAL, "%s: the chunk's last time %lld lies in baseline %lld, past n_base = %lld", who, (long long)(t1 - 1),
                    (long long)((t1 - 1) / len), (long long)n_base);
    if (__builtin_mul_overflow(n_det, n_chunk, &bc->n) || __builtin_mul_overflow(bc->n, (int64_t)16, &v))
        return fail(PXL_EINVAL, "%s: n_det * n_chunk overflows", who);
    if (__builtin_mul_overflow(n_det, n_base, &bc->nb) || __builtin_mul_overflow(bc->nb, (int64_t)8, &v))
        return fail(PXL_EINVAL, "%s: n_det * n_base overflows", who);
    if (!d && !a) return fail(PXL_EINVAL, "%s: d and a are both null", who);
    if (n_chunk > 0) { bc->b_lo = t0 / len; bc->nseg = (t1 - 1) / len - bc->b_lo + 1; }
    bc->small = bc->n < 0x7fffffffLL && t1 < 0x7fffffffLL && len < 0x7fffffffLL;
    return PXL_OK;
}

int pxl_baseline_bin_car_pol_nearest_f64(const pxl_car_wcs* wcs, const int64_t shape[3], double* rhs3, const double* mask, int64_t n_det,
                                         int64_t n_chunk, int64_t t0, int64_t baseline_len, int64_t n_base, const double* sky,
                                         const double* resp, const double* w, const double* d, const double* a, void* stream) {
    const char* who = "baseline_bin";
    BaselineCall bc;
    if (int rc = check_baselines(who, n_det, n_chunk, t0, baseline_len, n_base, d, a, &bc)) return rc;
    PointCall c(who, wcs, shape, bc.n, sky);
    c.polarised(resp).reads(w, 1);
    if (d) c.reads(d, 1);
    if (int rc = check_points(c.writes(rhs3, 3))) return rc;
    if (c.idle) return PXL_OK;
    const uintptr_t pb = (uintptr_t)(shape[1] * shape[0]) * 8;
    if (a && overlaps(rhs3, 3 * pb, a, (uintptr_t)bc.nb * 8)) return fail(PXL_EINVAL, "%s: rhs3 overlaps a", who);
    if (mask && overlaps(rhs3, 3 * pb, mask, pb)) return fail(PXL_EINVAL, "%s: rhs3 overlaps mask", who);
    return launch_points(c, "k_baseline_bin", k_baseline_bin, PXL_ZUNR, stream, rhs3, mask, shape[0], shape[1], car_periodic(wcs, shape[0]),
                         bc.n, n_chunk, t0, baseline_len, n_base, bc.small, (const double2*)sky, (const double2*)resp, w, d, a);
}

// project: one group of G lanes per (detector, baseline) segment of the chunk, G from baseline_len alone (pxl_baseline.h)
int pxl_baseline_project_car_pol_nearest_f64(const pxl_car_wcs* wcs, const int64_t shape[3], const double* map3, const double* mask,
                                             int64_t n_det, int64_t n_chunk, int64_t t0, int64_t baseline_len, int64_t n_base,
                                             const double* sky, const double* resp, const double* w, const double* d, const double* a,
                                             double* out, void* stream) {
    const char* who = "baseline_project";
    BaselineCall bc;
    if (int rc = check_baselines(who, n_det, n_chunk, t0, baseline_len, n_base, d, a, &bc)) return rc;
    PointCall c(who, wcs, shape, bc.n, sky);
    c.polarised(resp).reads(w, 1);
    if (d) c.reads(d, 1);
    if (int rc = check_points(c.needs(out))) return rc;
    if (c.idle) return PXL_OK;
    uintptr_t pb = 0;
    if (!range_bytes(shape[1], shape[0], 3, &pb)) return fail(PXL_EINVAL, "%s: sizes overflow", who);
    pb /= 3;
    const uintptr_t ob = (uintptr_t)bc.nb * 8, nb8 = (uintptr_t)bc.n * 8;
    if (overlaps(out, ob, sky, 2 * nb8) || overlaps(out, ob, resp, 2 * nb8) || overlaps(out, ob, w, nb8) || (d && overlaps(out, ob, d, nb8)) ||
        (a && overlaps(out, ob, a, ob)) || (map3 && overlaps(out, ob, map3, 3 * pb)) || (mask && overlaps(out, ob, mask, pb)))
        return fail(PXL_EINVAL, "%s: out overlaps the points, the responses, w, d, a, map3 or mask", who);
    int G = 256;                                                // a block per segment from 1024 samples on, else a power of two up to a wavefront
    if (baseline_len < 1024) for (G = 1; G < 64 && G < baseline_len; G *= 2) {}
    const int64_t nseg_all = n_det * bc.nseg;
    const Sky2Pix s = sky2pix_setup(*wcs, shape[0], shape[1], 1, PXL_FORM_RECIP);
    const dim3 grid(stream_grid(nseg_all, 256 / G));
    auto kern = baseline_len >= 1024 ? k_baseline_project<4> : baseline_len > 64 ? k_baseline_project<2> : k_baseline_project<1>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, s, map3, mask, shape[0], shape[1], car_periodic(wcs, shape[0]), n_chunk, t0,
                       baseline_len, n_base, bc.b_lo, bc.nseg, nseg_all, G, (const double2*)sky, (const double2*)resp, w, d, a, out);
    return check_launch("k_baseline_project");
}

// ---- the per-scan polynomial filter (pxl_polyfilter.h): every check before the first HIP call.
// G of k_polyfilter, from n_t, n_seg and the order alone: a block per segment where the mean segment has 1024 samples or more,
// else the power of two up to a wavefront that leaves a lane about order + 1 samples of a mean segment -- the tree costs a lane
// as much as a few samples do, and more so the more moments there are.
static int polyfilter_group(int64_t n_t, int64_t n_seg, int order) {
    const int64_t mean = n_t / (n_seg > 0 ? n_seg : 1);
    if (mean >= 1024) return 256;
    const int64_t lanes = (mean + order) / (order + 1);
    int G = 1;
    while (G < 64 && G < lanes) G *= 2;
    return G;
}

int pxl_tod_polyfilter_f64(int64_t n_det, int64_t n_t, int64_t n_seg, const int64_t* seg_start, int order, double rcond_min, const double* d,
                           const double* wfit, double* out, double* coeffs, int64_t* n_used, void* stream) {
    const char* who = "tod_polyfilter";
    if (order < 0 || order > 7) return fail(PXL_EINVAL, "%s: order must be 0 to 7 (got %d)", who, order);
    if (int rc = check_fit_rcond(who, rcond_min)) return rc;
    if (n_det < 0 || n_t < 0 || n_seg < 0)
        return fail(PXL_EINVAL, "%s: n_det, n_t and n_seg may not be negative (got %lld, %lld, %lld)", who, (long long)n_det, (long long)n_t,
                    (long long)n_seg);
    int64_t n, nf, nc, items, v;
    if (__builtin_mul_overflow(n_det, n_t, &n) || __builtin_mul_overflow(n, (int64_t)8, &v)) return fail(PXL_EINVAL, "%s: n_det * n_t overflows", who);
    if (n_seg > INT64_MAX / 8 - 2 || __builtin_mul_overflow(n_det, n_seg + 2, &items) || __builtin_mul_overflow(n_det, n_seg, &nf) ||
        __builtin_mul_overflow(nf, (int64_t)(order + 1), &nc) || __builtin_mul_overflow(nc, (int64_t)8, &v))
        return fail(PXL_EINVAL, "%s: n_det * n_seg overflows", who);
    if (n == 0) return PXL_OK;
    const uintptr_t nb = (uintptr_t)n * 8;
    const Span rd[3] = {{d, nb, "d"}, {wfit, wfit ? nb : 0, "wfit"}, {seg_start, (uintptr_t)(n_seg + 1) * 8, "seg_start"}};
    const Span wr[3] = {{out, nb, "out"}, {coeffs, coeffs ? (uintptr_t)nc * 8 : 0, "coeffs"}, {n_used, n_used ? (uintptr_t)nf * 8 : 0, "n_used"}};
    if (int rc = check_spans(who, wr, 3, rd, 3)) return rc;
    const int G = polyfilter_group(n_t, n_seg, order);
    const int64_t blocks = (items + 256 / G - 1) / (256 / G);
    if (blocks > 0x7fffffffLL) return fail(PXL_EINVAL, "%s: n_det * (n_seg + 2) too large for one launch", who);
    static constexpr decltype(&k_polyfilter<0>) kern[8] = {k_polyfilter<0>, k_polyfilter<1>, k_polyfilter<2>, k_polyfilter<3>,
                                                          k_polyfilter<4>, k_polyfilter<5>, k_polyfilter<6>, k_polyfilter<7>};
    launch_chunks(kern[order], blocks, 256, stream, n_t, n_seg, items, seg_start, rcond_min, G, d, wfit, out, coeffs, n_used);
    return check_launch("k_polyfilter");
}

// ---- the detector-mode filter (pxl_modefilter.h): every check before the first HIP call.
// C of k_modefilter, from n_t and n_grp alone: the wide tile of 64 time samples (four row phases, each a whole wavefront) where it
// alone makes two blocks for each of the 256 compute units, else the narrow one of 16 (sixteen row phases): four times the blocks,
// and a quarter of the detectors to each lane.
static int modefilter_tile(int64_t n_t, int64_t n_grp) {
    return n_grp * ((n_t + 63) / 64) >= 512 ? 64 : 16;                      // n_grp * n_t does not overflow: checked by the caller
}

int pxl_tod_modefilter_f64(int64_t n_det, int64_t n_t, int64_t n_grp, const int64_t* grp_start, int n_modes, const double* modes, double rcond_min,
                           const double* d, const double* wfit, double* out, double* amps, int64_t* n_used, void* stream) {
    const char* who = "tod_modefilter";
    if (n_modes < 1 || n_modes > 8) return fail(PXL_EINVAL, "%s: n_modes must be 1 to 8 (got %d)", who, n_modes);
    if (int rc = check_fit_rcond(who, rcond_min)) return rc;
    if (n_det < 0 || n_t < 0 || n_grp < 0)
        return fail(PXL_EINVAL, "%s: n_det, n_t and n_grp may not be negative (got %lld, %lld, %lld)", who, (long long)n_det, (long long)n_t,
                    (long long)n_grp);
    int64_t n, nm, nf, na, v;
    if (__builtin_mul_overflow(n_det, n_t, &n) || __builtin_mul_overflow(n, (int64_t)8, &v)) return fail(PXL_EINVAL, "%s: n_det * n_t overflows", who);
    if (__builtin_mul_overflow(n_det, (int64_t)n_modes, &nm) || __builtin_mul_overflow(nm, (int64_t)8, &v))
        return fail(PXL_EINVAL, "%s: n_det * n_modes overflows", who);
    if (n_grp > INT64_MAX / 8 - 2 || __builtin_mul_overflow(n_grp, n_t, &nf) || __builtin_mul_overflow(nf, (int64_t)n_modes, &na) ||
        __builtin_mul_overflow(na, (int64_t)8, &v))
        return fail(PXL_EINVAL, "%s: n_grp * n_t overflows", who);
    if (n == 0) return PXL_OK;
    const uintptr_t nb = (uintptr_t)n * 8;
    const Span rd[4] = {{d, nb, "d"}, {wfit, wfit ? nb : 0, "wfit"}, {grp_start, (uintptr_t)(n_grp + 1) * 8, "grp_start"}, {modes, (uintptr_t)nm * 8, "modes"}};
    const Span wr[3] = {{out, nb, "out"}, {amps, amps ? (uintptr_t)na * 8 : 0, "amps"}, {n_used, n_used ? (uintptr_t)nf * 8 : 0, "n_used"}};
    if (int rc = check_spans(who, wr, 3, rd, 4)) return rc;
    const int C = modefilter_tile(n_t, n_grp);
    const int64_t tiles = (n_t + C - 1) / C;
    int64_t blocks;
    if (__builtin_mul_overflow(n_grp + 2, tiles, &blocks) || blocks > 0x7fffffffLL)
        return fail(PXL_EINVAL, "%s: (n_grp + 2) * ceil(n_t / %d) blocks are too many for one launch", who, C);
    static constexpr decltype(&k_modefilter<1>) kern[8] = {k_modefilter<1>, k_modefilter<2>, k_modefilter<3>, k_modefilter<4>,
                                                          k_modefilter<5>, k_modefilter<6>, k_modefilter<7>, k_modefilter<8>};
    launch_chunks(kern[n_modes - 1], blocks, 256, stream, n_det, n_t, n_grp, tiles, grp_start, modes, rcond_min, C, d, wfit, out, amps, n_used);
    return check_launch("k_modefilter");
}

// ---- the binned-template filter (pxl_binfilter.h): every check before the first HIP call.  G of k_binfilter is
// polyfilter_group's at order 0, from n_t and n_bin alone: a mean bin is a mean segment.
int pxl_tod_binfilter_f64(int64_t n_det, int64_t n_t, int64_t n_bin, const int64_t* bin_start, const int64_t* order, const double* d,
                          const double* wfit, double* out, double* means, int64_t* n_used, void* stream) {
    const char* who = "tod_binfilter";
    if (n_det < 0 || n_t < 0 || n_bin < 0)
        return fail(PXL_EINVAL, "%s: n_det, n_t and n_bin may not be negative (got %lld, %lld, %lld)", who, (long long)n_det, (long long)n_t,
                    (long long)n_bin);
    int64_t n, nf, items, v;
    if (__builtin_mul_overflow(n_det, n_t, &n) || __builtin_mul_overflow(n, (int64_t)8, &v)) return fail(PXL_EINVAL, "%s: n_det * n_t overflows", who);
    if (n_bin > INT64_MAX / 8 - 2 || __builtin_mul_overflow(n_det, n_bin + 2, &items) || __builtin_mul_overflow(n_det, n_bin, &nf) ||
        __builtin_mul_overflow(nf, (int64_t)8, &v))
        return fail(PXL_EINVAL, "%s: n_det * n_bin overflows", who);
    if (n == 0) return PXL_OK;
    const uintptr_t nb = (uintptr_t)n * 8, fb = (uintptr_t)nf * 8;
    const Span rd[4] = {{d, nb, "d"}, {wfit, wfit ? nb : 0, "wfit"}, {bin_start, (uintptr_t)(n_bin + 1) * 8, "bin_start"},
                        {order, (uintptr_t)n_t * 8, "order"}};
    const Span wr[3] = {{out, nb, "out"}, {means, means ? fb : 0, "means"}, {n_used, n_used ? fb : 0, "n_used"}};
    if (int rc = check_spans(who, wr, 3, rd, 4)) return rc;
    const int G = polyfilter_group(n_t, n_bin, 0);
    const int64_t blocks = (items + 256 / G - 1) / (256 / G);
    if (blocks > 0x7fffffffLL) return fail(PXL_EINVAL, "%s: n_det * (n_bin + 2) too large for one launch", who);
    launch_chunks(k_binfilter, blocks, 256, stream, n_det, n_t, n_bin, items, bin_start, order, G, d, wfit, out, means, n_used);
    return check_launch("k_binfilter");
}

// ---- the banded-Toeplitz noise weight (pxl_toeplitz.h): every check before the first HIP call.  The instantiation
// follows lambda alone: the size of the LDS, and from lambda = 17 on the sliding windows; the tile is PXL_TOEP_C samples at every lambda.
int pxl_tod_toeplitz_f64(int64_t n_det, int64_t n_t, int64_t n_seg, const int64_t* seg_start, int64_t lambda, const double* kern,
                         const double* x, const double* wlive, double* out, void* stream) {
    const char* who = "tod_toeplitz";
    if (lambda < 0 || lambda > 4096) return fail(PXL_EINVAL, "%s: lambda must be 0 to 4096 (got %lld)", who, (long long)lambda);
    if (n_det < 0 || n_t < 0 || n_seg < 0)
        return fail(PXL_EINVAL, "%s: n_det, n_t and n_seg may not be negative (got %lld, %lld, %lld)", who, (long long)n_det, (long long)n_t,
                    (long long)n_seg);
    int64_t n, nk, v;
    if (__builtin_mul_overflow(n_det, n_t, &n) || __builtin_mul_overflow(n, (int64_t)8, &v)) return fail(PXL_EINVAL, "%s: n_det * n_t overflows", who);
    if (__builtin_mul_overflow(n_det, lambda + 1, &nk) || __builtin_mul_overflow(nk, (int64_t)8, &v))
        return fail(PXL_EINVAL, "%s: n_det * (lambda + 1) overflows", who);
    if (n_seg > INT64_MAX / 8 - 2) return fail(PXL_EINVAL, "%s: the bytes of n_seg + 1 offsets overflow", who);
    if (n == 0) return PXL_OK;
    const uintptr_t nb = (uintptr_t)n * 8;
    // an output reads its neighbours, so there is no in-place form: check_spans' in-place pair is (out, nothing), and x is read like the rest
    const Span rd[5] = {{nullptr, 0, ""}, {x, nb, "x"}, {kern, (uintptr_t)nk * 8, "kern"}, {seg_start, (uintptr_t)(n_seg + 1) * 8, "seg_start"},
                        {wlive, wlive ? nb : 0, "wlive"}};
    const Span wr[1] = {{out, nb, "out"}};
    if (int rc = check_spans(who, wr, 1, rd, 5)) return rc;
    const int64_t tiles = (n_t + PXL_TOEP_C - 1) / PXL_TOEP_C;
    int64_t blocks;
    if (__builtin_mul_overflow(n_det, tiles, &blocks) || blocks > 0x7fffffffLL)
        return fail(PXL_EINVAL, "%s: n_det * ceil(n_t / %d) blocks are too many for one launch", who, PXL_TOEP_C);
    auto k = lambda <= 16 ? k_toeplitz<128, false> : lambda <= 128 ? k_toeplitz<128, true> : lambda <= 1024 ? k_toeplitz<1024, true> : k_toeplitz<4096, true>;
    launch_chunks(k, blocks, 256, stream, n_t, n_seg, tiles, seg_start, (int)lambda, kern, x, wlive, out);
    return check_launch("k_toeplitz");
}

// ---- the gappy autocovariance (pxl_autocov.h): every check before the first HIP call.  The lanes of a group, and
// with them the order of the sum, follow lambda alone; both outputs are overwritten, so with no samples they are still zeroed.
int pxl_tod_autocov_f64(int64_t n_det, int64_t n_t, int64_t n_seg, const int64_t* seg_start, int64_t lambda, const double* x,
                        const double* wlive, double* sums, int64_t* pairs, void* stream) {
    const char* who = "tod_autocov";
    if (lambda < 0 || lambda > 4096) return fail(PXL_EINVAL, "%s: lambda must be 0 to 4096 (got %lld)", who, (long long)lambda);
    if (n_det < 0 || n_t < 0 || n_seg < 0)
        return fail(PXL_EINVAL, "%s: n_det, n_t and n_seg may not be negative (got %lld, %lld, %lld)", who, (long long)n_det, (long long)n_t,
                    (long long)n_seg);
    int64_t n, nk, v;
    if (__builtin_mul_overflow(n_det, n_t, &n) || __builtin_mul_overflow(n, (int64_t)8, &v)) return fail(PXL_EINVAL, "%s: n_det * n_t overflows", who);
    if (__builtin_mul_overflow(n_det, lambda + 1, &nk) || __builtin_mul_overflow(nk, (int64_t)8, &v))
        return fail(PXL_EINVAL, "%s: n_det * (lambda + 1) overflows", who);
    if (n_seg > INT64_MAX / 8 - 2) return fail(PXL_EINVAL, "%s: the bytes of n_seg + 1 offsets overflow", who);
    if (nk == 0) return PXL_OK;
    const uintptr_t nb = (uintptr_t)n * 8, kb = (uintptr_t)nk * 8;
    // nothing is in place: check_spans' in-place pair is (sums, nothing).  With no samples only the outputs have bytes.
    const Span rd[4] = {{nullptr, 0, ""}, {x, nb, "x"}, {seg_start, n ? (uintptr_t)(n_seg + 1) * 8 : 0, "seg_start"}, {wlive, wlive ? nb : 0, "wlive"}};
    const Span wr[2] = {{sums, n || sums ? kb : 0, "sums"}, {pairs, pairs ? kb : 0, "pairs"}};
    if (int rc = check_spans(who, wr, 2, rd, 4)) return rc;
    if (n == 0) {
        if (sums) HIP_TRY(hipMemsetAsync(sums, 0, kb, (hipStream_t)stream));
        if (pairs) HIP_TRY(hipMemsetAsync(pairs, 0, kb, (hipStream_t)stream));
        return PXL_OK;
    }
    const int lpg = autocov_lpg_log2(lambda);
    const int64_t n_grp = (lambda + (5 << lpg)) / (5 << lpg);
    int64_t blocks;
    if (__builtin_mul_overflow(n_det, n_grp, &blocks) || blocks > 0x7fffffffLL)
        return fail(PXL_EINVAL, "%s: n_det * ceil((lambda + 1) / %d) blocks are too many for one launch", who, 5 << lpg);
    launch_chunks(k_autocov, blocks, 256, stream, n_t, n_seg, (int)n_grp, seg_start, (int)lambda, lpg, x, wlive, sums, pairs);
    return check_launch("k_autocov");
}

// ---- the per-pixel IQU block solve and product (pxl_polsolve.h) ----------------------------------------------
// what the two entries share: sizes, pointers, and the ranges that may not meet.  in3 is the right-hand side (solve) or x (apply):
// out3 may be exactly in3, and nothing else may overlap anything written.  rcond is null for apply.
static int check_polsolve(const char* who, const double* w6, const double* in3, const double* out3, const double* rcond, int64_t npix) {
    if (npix < 0) return fail(PXL_EINVAL, "%s: negative npix", who);
    if (npix == 0) return PXL_OK;
    if (!w6 || !in3 || !out3) return fail(PXL_EINVAL, "%s: null buffer", who);
    if (npix > INT64_MAX / 48) return fail(PXL_EINVAL, "%s: sizes overflow", who);
    if ((((uintptr_t)w6 | (uintptr_t)in3 | (uintptr_t)out3 | (uintptr_t)rcond) & 7) != 0)
        return fail(PXL_EINVAL, "%s: buffers must be 8-byte aligned", who);
    const uintptr_t nb = (uintptr_t)npix * 8;
    if (overlaps(out3, 3 * nb, w6, 6 * nb)) return fail(PXL_EINVAL, "%s: out overlaps the weights", who);
    if (out3 != in3 && overlaps(out3, 3 * nb, in3, 3 * nb)) return fail(PXL_EINVAL, "%s: out overlaps its input other than exactly (in place)", who);
    if (rcond && (overlaps(rcond, nb, out3, 3 * nb) || overlaps(rcond, nb, w6, 6 * nb) || overlaps(rcond, nb, in3, 3 * nb)))
        return fail(PXL_EINVAL, "%s: rcond overlaps out or an input", who);
    return PXL_OK;
}
// two pixels per lane when every plane of every buffer starts on a 16-byte boundary: plane c starts c * npix * 8 bytes in
static bool polsolve_vec(int64_t npix, const void* a, const void* b, const void* c, const void* d) {
    return (npix % 2 == 0) && ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0);
}

int pxl_pol_block_solve_f64(const double* weights6, const double* rhs3, double* out3, double* rcond, int64_t npix, double rcond_min,
                            void* stream) {
    if (!std::isfinite(rcond_min) || !(rcond_min > 0.0) || rcond_min > 1.0)
        return fail(PXL_EINVAL, "pol_block_solve: rcond_min must lie in (0, 1] (got %g)", rcond_min);
    if (int rc = check_polsolve("pol_block_solve", weights6, rhs3, out3, rcond, npix)) return rc;
    if (npix == 0) return PXL_OK;
    const bool vec = polsolve_vec(npix, weights6, rhs3, out3, rcond);
    const int64_t items = vec ? npix / 2 : npix;
    auto kern = vec ? (rcond ? k_pol_block_solve<true, true> : k_pol_block_solve<true, false>)
                    : (rcond ? k_pol_block_solve<false, true> : k_pol_block_solve<false, false>);
    hipLaunchKernelGGL(kern, dim3(stream_grid(items, 256)), dim3(256), 0, (hipStream_t)stream, weights6, rhs3, out3, rcond, npix, items,
                       rcond_min);
    return check_launch("k_pol_block_solve");
}

int pxl_pol_block_apply_f64(const double* weights6, const double* x3, double* out3, int64_t npix, void* stream) {
    if (int rc = check_polsolve("pol_block_apply", weights6, x3, out3, nullptr, npix)) return rc;
    if (npix == 0) return PXL_OK;
    const bool vec = polsolve_vec(npix, weights6, x3, out3, nullptr);
    const int64_t items = vec ? npix / 2 : npix;
    auto kern = vec ? k_pol_block_apply<true> : k_pol_block_apply<false>;
    hipLaunchKernelGGL(kern, dim3(stream_grid(items, 256)), dim3(256), 0, (hipStream_t)stream, weights6, x3, out3, npix, items);
    return check_launch("k_pol_block_apply");
}

// ---- detector pointing expansion (pxl_pointing.h): every check before the first HIP call
int pxl_pointing_expand_f64(int64_t nt, const double* qbore_4xT, int64_t nd, const double* qdet_4xD, const double* gamma_D, double* sky2xN,
                            double* resp2xN, void* stream) {
    if (nt < 0 || nd < 0) return fail(PXL_EINVAL, "pointing_expand: negative %s", nt < 0 ? "nt" : "nd");
    if (nt > 0 && nd > INT64_MAX / 32 / nt) return fail(PXL_EINVAL, "pointing_expand: nd * nt overflows");
    const int64_t n = nd * nt;
    if (n == 0) return PXL_OK;
    if (!qbore_4xT || !qdet_4xD || !sky2xN || !resp2xN)
        return fail(PXL_EINVAL, "pointing_expand: null %s", !qbore_4xT ? "qbore" : !qdet_4xD ? "qdet" : !sky2xN ? "sky" : "resp");
    if (((uintptr_t)qbore_4xT & 15) != 0) return fail(PXL_EINVAL, "pointing_expand: qbore must be 16-byte aligned");
    if (((uintptr_t)sky2xN & 15) != 0) return fail(PXL_EINVAL, "pointing_expand: sky must be 16-byte aligned");
    if (((uintptr_t)resp2xN & 15) != 0) return fail(PXL_EINVAL, "pointing_expand: resp must be 16-byte aligned");
    if ((((uintptr_t)qdet_4xD | (uintptr_t)gamma_D) & 7) != 0) return fail(PXL_EINVAL, "pointing_expand: qdet and gamma must be 8-byte aligned");
    const uintptr_t ob = (uintptr_t)n * 16;
    const char* who = "pointing_expand";
    const Span sky = {sky2xN, ob, "sky"}, resp = {resp2xN, ob, "resp"};
    const Span rd[3] = {{qbore_4xT, (uintptr_t)nt * 32, "qbore"}, {qdet_4xD, (uintptr_t)nd * 32, "qdet"}, {gamma_D, gamma_D ? (uintptr_t)nd * 8 : 0, "gamma"}};
    for (const Span& r : rd) {
        if (int rc = check_apart(who, sky, r)) return rc;
        if (int rc = check_apart(who, resp, r)) return rc;
    }
    if (int rc = check_apart(who, sky, resp)) return rc;
    const int64_t ntb = (nt + PXL_PT_BLOCK - 1) / PXL_PT_BLOCK, ndg = (nd + PXL_PT_GROUP - 1) / PXL_PT_GROUP;
    if (ntb > 0x7fffffffLL / ndg) return fail(PXL_EINVAL, "pointing_expand: nd * nt too large for one launch");
    launch_chunks(k_pointing_expand, ntb * ndg, PXL_PT_BLOCK, stream, nt, nd, (unsigned)ntb, (const double2*)qbore_4xT, qdet_4xD, gamma_D,
                  (double2*)sky2xN, (double2*)resp2xN);
    return check_launch("k_pointing_expand");
}

// ---- row-pair layout (pxl_sample.h): caller-owned buffer of pxl_sample_pairs_elems() map elements
int64_t pxl_sample_pairs_elems(const int64_t shape_in[3], int64_t src_nrows) {
    if (!shape_in || shape_in[0] < 1 || shape_in[1] < 1 || shape_in[2] < 1 || src_nrows < 0 || src_nrows > shape_in[1]) {
        fail(PXL_EINVAL, "sample_pairs_elems: invalid shape or window");
        return -1;
    }
    // one size for both element types: Float64 rows (groups of 4 entries, 3 new columns each) are the longer ones except
    // on maps of a few columns, where the rounding up to whole groups can favour Float32 (8 entries, 7 new columns)
    const int64_t e64 = PairGroup<double>::groups(shape_in[0]) * PairGroup<double>::E;
    const int64_t e32 = PairGroup<float>::groups(shape_in[0]) * PairGroup<float>::E;
    return 2 * (e64 > e32 ? e64 : e32) * (src_nrows + 1) * shape_in[2];
}

int pxl_sample_build_pairs_f64(const int64_t shape_in[3], const double* src, int64_t src_nrows, double* pairs, void* stream) {
    return build_pairs_impl(shape_in, src, src_nrows, pairs, stream);
}

int pxl_sample_build_pairs_f32(const int64_t shape_in[3], const float* src, int64_t src_nrows, float* pairs, void* stream) {
    return build_pairs_impl(shape_in, src, src_nrows, pairs, stream);
}

int pxl_sample_car_bilinear_pairs_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* pairs,
                                      int64_t src_row0, int64_t src_nrows, int64_t n, const double* sky, double* out,
                                      void* stream) {
    return sample_pairs_impl(wcs_in, shape_in, pairs, src_row0, src_nrows, n, sky, out, stream);
}

int pxl_sample_car_bilinear_pairs_f32(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const float* pairs,
                                      int64_t src_row0, int64_t src_nrows, int64_t n, const double* sky, float* out,
                                      void* stream) {
    return sample_pairs_impl(wcs_in, shape_in, pairs, src_row0, src_nrows, n, sky, out, stream);
}

int pxl_fits_decode_f64(const void* raw_be, double* dst, int64_t n, int bitpix, void* stream) {
    if (n < 0 || (n > 0 && (!raw_be || !dst))) return fail(PXL_EINVAL, "fits_decode: null buffer or negative n");
    if (bitpix != -64 && bitpix != -32) return fail(PXL_EINVAL, "fits_decode: BITPIX %d not supported (only -64, -32)", bitpix);
    if (n == 0) return PXL_OK;
    hipLaunchKernelGGL(k_bswap_to_f64, dim3(stream_grid((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, raw_be, dst, n, bitpix);
    return check_launch("k_bswap_to_f64");
}

int pxl_fits_swap_f32(const void* src, void* dst, int64_t n, void* stream) {
    if (n < 0 || (n > 0 && (!src || !dst))) return fail(PXL_EINVAL, "fits_swap_f32: null buffer or negative n");
    if (n == 0) return PXL_OK;
    hipLaunchKernelGGL(k_bswap32, dim3(stream_grid((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint32_t*)src, (uint32_t*)dst, n);
    return check_launch("k_bswap32");
}

int pxl_fits_encode_f64(const double* src, void* raw_be, int64_t n, void* stream) {
    if (n < 0 || (n > 0 && (!raw_be || !src))) return fail(PXL_EINVAL, "fits_encode: null buffer or negative n");
    if (n == 0) return PXL_OK;
    hipLaunchKernelGGL(k_f64_to_be, dim3(stream_grid((n + 3) / 4, 256)), dim3(256), 0, (hipStream_t)stream, src, (uint64_t*)raw_be, n);
    return check_launch("k_f64_to_be");
}

int pxl_fill_random_f64(double* dst, int64_t n, uint64_t seed, uint64_t offset, int kind, void* stream) {
    if (n < 0 || (n > 0 && !dst)) return fail(PXL_EINVAL, "fill_random: null buffer or negative n");
    if (n == 0) return PXL_OK;
    hipLaunchKernelGGL(k_fill_random, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, dst, n, seed,
                       offset, kind);
    return check_launch("k_fill_random");
}

int pxl_fill_sphere_points_f64(double* sky, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
    if (n < 0 || (n > 0 && !sky)) return fail(PXL_EINVAL, "fill_sphere: null buffer or negative n");
    if (((uintptr_t)sky & 15) != 0) return fail(PXL_EINVAL, "fill_sphere: 2xN buffer must be 16-byte aligned");
    if (n == 0) return PXL_OK;
    hipLaunchKernelGGL(k_fill_sphere, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, (double2*)sky,
                       n, seed, offset);
    return check_launch("k_fill_sphere");
}

}  // extern "C"
