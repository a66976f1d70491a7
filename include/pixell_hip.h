/*
 * pixell_hip.h -- C ABI of libpixell_hip.so: MI355X (gfx950) kernels for the Pixell.jl CAR
 * pixel<->sky hot path (pix2sky / sky2pix evaluators, posmap, CAR->CAR bilinear reprojection and
 * scattered bilinear sampling, Float64).
 *
 * This is the drop-in boundary.  The reference (pure Julia) has no plugin ABI of its own; each entry
 * below names the reference method it replaces (file:line under /root/reference/src/).  A Julia host
 * binds these with `ccall((:sym, libpixell_hip), Cint, (...), ...)` in the style the reference already
 * uses for libsharp/wcslib (transforms.jl:185-194, arbitrary_wcs.jl:41-43); see INTEGRATION.md.
 *
 * Conventions
 *   - Plain C types only.  All data pointers are DEVICE pointers (HBM) unless named host_*.
 *   - Every entry returns 0 on success or a negative code (PXL_E*); it never throws, exits or prints.
 *     pxl_last_error() returns the thread-local message of the last failing call.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Entries only enqueue work;
 *     they never synchronise, allocate or free caller-visible memory (plans own their own tables).
 *   - Arrays are Julia column-major: maps are (nx, ny[, nc]) with RA the contiguous axis; coordinate
 *     batches are 2xN, i.e. interleaved (c1, c2) pairs (car_proj.jl:102-107).  Pixel coordinates are
 *     1-based Float64, angles are radians.
 *   - Arithmetic is IEEE double with NO fma contraction, written op-for-op from the reference's source.
 *     What is TESTED: results are bit-identical to the CPU oracle (oracle/pixell_oracle.c); the oracle matches
 *     every literal / data file of the reference's own tests at the reference's own tolerances (isapprox,
 *     100 eps).  The reference itself (Julia) has never been executed next to this library: DESIGN.md 7.
 */
#ifndef PIXELL_HIP_H
#define PIXELL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PXL_VERSION 100   /* 0.1.0 */

/* CarClenshawCurtis{Float64} / CarFejer1{Float64}: projections/car_proj.jl:7-19 (isbits, 56 bytes).
 * Also used for Gnomonic{Float64} (projections/tan_proj.jl:4-9), which has the same fields. */
typedef struct pxl_car_wcs {
    double cdelt[2];
    double crpix[2];
    double crval[2];
    double unit;      /* conversion factor to radians; pi/180 for degree WCS (enmap_geom.jl:18) */
} pxl_car_wcs;

/* error codes */
#define PXL_OK         0
#define PXL_EINVAL   (-22)   /* bad argument (null pointer, negative size, window outside the map) */
#define PXL_ENOMEM   (-12)   /* device allocation failed (plan creation only) */
#define PXL_EHIP     (-5)    /* a HIP runtime call failed; message has hipGetErrorString */
#define PXL_ENODEV   (-19)   /* no gfx950 device / kernel image not loadable */

/* `safe` keyword of the reference's array evaluators */
#define PXL_WRAP_NONE    0   /* safe=false */
#define PXL_WRAP_REWIND  1   /* per-element rewind (what scalar pix2sky does, car_proj.jl:148-150) */
#define PXL_WRAP_UNWIND  2   /* safe=true on 2xN arrays: rewind then unwrap along N (car_proj.jl:110-112) */

/* the reference's three sky2pix roundings (they differ in the last bit) */
#define PXL_FORM_RECIP     0 /* sky2pix!(2xN):      i0 + (a-a0)*(1/d), period abs(2pi/d)      car_proj.jl:165-193 */
#define PXL_FORM_DIV       1 /* sky2pix(ra, dec):   i0 + (a-a0)/d,     period abs(2pi/d)      car_proj.jl:220-234 */
#define PXL_FORM_RECIP_AV  2 /* sky2pix(ras, decs): i0 + (a-a0)*(1/d), period abs(2pi*(1/d))  car_proj.jl:235-252 */

int         pxl_version(void);
/* copies the calling thread's last error message (NUL-terminated, truncated to n) and returns its length */
size_t      pxl_last_error(char* buf, size_t n);
/* number of visible HIP devices, or a negative error */
int         pxl_device_count(void);
/* unwind (safe=true on 2xN batches) takes its scratch (10 bytes per coordinate) from a library-owned stream-ordered
 * pool on the current device and keeps it between calls; this returns the unused part to the driver */
int         pxl_release_scratch(void);

/* ---- pix2sky!(shape, wcs::AbstractCARWCS, pixcoords::2xN, skycoords::2xN; safe)   car_proj.jl:92-115
 *      In-place (pix == sky) is allowed; partially overlapping buffers are refused (PXL_EINVAL) in _UNWIND mode.
 *      wrap_mode: PXL_WRAP_NONE | _REWIND | _UNWIND.  _UNWIND handles at most 2^31-1 points per call.     */
int pxl_pix2sky_car_f64(const pxl_car_wcs* wcs, int64_t n, const double* pix2xN, double* sky2xN,
                        int wrap_mode, void* stream);

/* ---- rewind!(angles; period, ref_angle)                                            enmap_ops.jl:15-19
 *      unwind!(angles; dims, period, ref_angle)                                      enmap_ops.jl:26-32
 *      rewind is elementwise over n doubles.  unwind works along the point axis of an nrow x N column-major
 *      array (nrow = 2: a 2xN coordinate batch with dims=2; nrow = 1: a plain vector), in place.           */
int pxl_rewind_f64(double* a, int64_t n, double period, double ref_angle, void* stream);
int pxl_unwind_f64(double* a, int64_t n, int nrow, double period, double ref_angle, void* stream);

/* ---- pix2sky(shape, wcs, ra_pixel, dec_pixel; safe) broadcast over two N-vectors   car_proj.jl:141-152
 *      safe != 0 -> rewind(ra), rewind(dec).                                                         */
int pxl_pix2sky_car_soa_f64(const pxl_car_wcs* wcs, int64_t n, const double* ipix, const double* jpix,
                            double* ra, double* dec, int safe, void* stream);

/* ---- sky2pix!(shape, wcs, skycoords::2xN, pixcoords::2xN; safe)                    car_proj.jl:165-193
 *      form = PXL_FORM_RECIP reproduces it bit-for-bit; the other forms are exposed for completeness. */
int pxl_sky2pix_car_f64(const pxl_car_wcs* wcs, const int64_t shape[2], int64_t n, const double* sky2xN,
                        double* pix2xN, int safe, int form, void* stream);

/* ---- sky2pix(shape, wcs, ra::AV, dec::AV; safe)   (form = PXL_FORM_RECIP_AV)        car_proj.jl:235-252
 *      sky2pix(shape, wcs, ra::Number, dec::Number) broadcast (form = PXL_FORM_DIV)   car_proj.jl:220-234 */
int pxl_sky2pix_car_soa_f64(const pxl_car_wcs* wcs, const int64_t shape[2], int64_t n, const double* ra,
                            const double* dec, double* ipix, double* jpix, int safe, int form, void* stream);

/* ---- posmap(shape, wcs)                                                             enmap_ops.jl:190-203
 *      Writes rows [row0, row0+nrows) (0-based) of the (nx, ny) RA and DEC maps; ra/dec each hold
 *      nx*nrows doubles.  The reference always uses safe=true (scalar pix2sky -> rewind).             */
int pxl_posmap_car_f64(const pxl_car_wcs* wcs, const int64_t shape[2], int64_t row0, int64_t nrows,
                       double* ra, double* dec, int safe, void* stream);

/* ---- pixareamap!(pixareas)                                                          enmap_ops.jl:124-138
 *      Fills rows [row0, row0+nrows) of an (nx, ny) map with the per-row pixel area (steradians).     */
int pxl_pixareamap_car_f64(const pxl_car_wcs* wcs, const int64_t shape[2], int64_t row0, int64_t nrows,
                           double* area, void* stream);

/* ---- distance_transform(::AbstractSDT, m)                                   transform_distance.jl:55-78, :193-203, :322-344
 *      For every pixel of the (nx, ny) map m, the angular distance (radians) to the nearest pixel whose value is zero
 *      (m == 0.0, Julia's iszero: -0.0 counts, NaN does not), written to dist (nx, ny).  Exact, like BruteForceSDT: the
 *      nearest zero is found in O(nx * ny) work whatever the mask (a scan per row, then a convex chain and a sweep per
 *      column), and its distance is evaluated as the reference does, acos(1 - d^2/2) with d^2 from the pixel
 *      centres' cos / sin tables in the difference form of `metric` (transform_distance.jl:81-92).  A zero pixel gets
 *      exactly 0.0.  Deviation from the reference: the tables come from the device's cos / sin, and a near-tie between two
 *      zeros may be resolved the other way; each pixel is within a few eps / sin(theta) of the reference.
 *      That bound assumes cos DEC >= 0 on every row, i.e. |DEC| <= Float64(pi/2), which full-sky CC pole rows meet exactly.
 *      Rows up to 1e-9 beyond a pole are accepted, but a row e beyond it may add up to 4e to the error in d^2.
 *      No zero in the map: every output is +Inf (the reference's acos throws DomainError there; the host wrappers do).
 *      Full 2-D maps, nx <= 131072.  Scratch: 12 bytes per pixel plus 16 per row and column, from the library's
 *      stream-ordered pool (pxl_release_scratch); asynchronous on `stream`, no host synchronisation.
 *      PXL_EINVAL before any device work: an invalid WCS or shape, a null pointer, dist overlapping m, a map wider than
 *      360 degrees of RA, or a row with |DEC| > pi/2 + 1e-9.                    */
int pxl_distance_transform_car_f64(const pxl_car_wcs* wcs, const int64_t shape[2], const double* m,
                                   double* dist, void* stream);

/* ---- Gnomonic evaluators over N-vectors                                             tan_proj.jl:44-75
 *      (the reference has scalar methods only; posmap(shape, ::Gnomonic) loops them).                 */
int pxl_sky2pix_tan_f64(const pxl_car_wcs* wcs, int64_t n, const double* ra, const double* dec,
                        double* ipix, double* jpix, void* stream);
int pxl_pix2sky_tan_f64(const pxl_car_wcs* wcs, int64_t n, const double* ipix, const double* jpix,
                        double* ra, double* dec, void* stream);
int pxl_posmap_tan_f64(const pxl_car_wcs* wcs, const int64_t shape[2], int64_t row0, int64_t nrows,
                       double* ra, double* dec, void* stream);

/* ---- Bilinear reprojection CAR -> CAR.  NOT in the reference: the composite
 *      posmap(out) [enmap_ops.jl:190-203, safe=false] o sky2pix(in) [car_proj.jl:220-234, safe=true]
 *      o 2x2 gather + lerp, defined by oracle/pixell_oracle.c.
 *
 *      A plan holds the separable coordinate tables (nx_out + ny_out entries) in device memory.
 *      src holds rows [src_row0, src_row0+src_nrows) of every component plane of the (nx, ny, nc)
 *      source map: (nx, src_nrows, nc) column-major; dst receives rows [dst_row0, dst_row0+dst_nrows)
 *      of the (nx_out, ny_out, nc) output: (nx_out, dst_nrows, nc).  Full maps: row0 = 0, nrows = ny.
 *      Windows are how a declination strip (+ halo rows) of a sharded map is described without
 *      changing a single bit of the coordinate arithmetic.                                          */
typedef struct pxl_reproject_plan pxl_reproject_plan;

int pxl_reproject_plan_create(const pxl_car_wcs* wcs_in, const int64_t shape_in[3],
                              int64_t src_row0, int64_t src_nrows,
                              const pxl_car_wcs* wcs_out, const int64_t shape_out[2],
                              int64_t dst_row0, int64_t dst_nrows,
                              pxl_reproject_plan** plan);
/* enqueue table build + reprojection of all nc components on `stream` */
int pxl_reproject_execute(pxl_reproject_plan* plan, const double* src, double* dst, void* stream);
/* as above but only output rows [r0, r0+nr) RELATIVE to the plan's dst window (for interior/boundary
 * splitting while a halo is in flight); the tables must have been built by a previous execute/build ON THE
 * SAME STREAM (or one the caller has ordered before this one).  A plan may be shared by host threads only
 * for concurrent execute_rows calls; create/build/destroy are the owner's.  src and dst must not overlap.
 * Tuning knobs read once at plan creation: PXL_REPROJECT_{RH,PAIRS,NS,PF,NT}.             */
int pxl_reproject_build_tables(pxl_reproject_plan* plan, void* stream);
int pxl_reproject_execute_rows(pxl_reproject_plan* plan, const double* src, double* dst,
                               int64_t r0, int64_t nr, void* stream);
/* Float32 maps (Enmap{Float32}: the storage type most released maps use).  Same plan, same Float64 coordinate
 * tables and weights; taps are widened to Float64, the result is rounded once to Float32 -- what Julia does when
 * a Float64 expression is assigned into a Float32 array.                                                        */
int pxl_reproject_execute_f32(pxl_reproject_plan* plan, const float* src, float* dst, void* stream);
int pxl_reproject_execute_rows_f32(pxl_reproject_plan* plan, const float* src, float* dst,
                                   int64_t r0, int64_t nr, void* stream);
/* source rows [lo, hi) (0-based, absolute) that the plan's dst window reads (host computation,
 * same arithmetic as the device tables) -- what a shard must hold, i.e. strip + halo.               */
int pxl_reproject_plan_src_rows(const pxl_reproject_plan* plan, int64_t* lo, int64_t* hi);
/* output rows (relative to the dst window, [lo, hi)) whose stencil lies entirely inside source rows
 * [have_lo, have_hi) -- the interior that can start before a halo arrives.                           */
int pxl_reproject_plan_rows_covered(const pxl_reproject_plan* plan, int64_t have_lo, int64_t have_hi,
                                    int64_t* lo, int64_t* hi);
/* tuning knob for benchmarking / cross-checks: 0 = auto (LDS-DMA kernel when the source allows 16-B loads),
 * 1 = direct-gather kernel, 2 = register-staged kernel */
int pxl_reproject_plan_set_variant(pxl_reproject_plan* plan, int variant);
int pxl_reproject_plan_destroy(pxl_reproject_plan* plan);

/* ---- One step of the dec-strip sharded operator on this rank: exchange halo rows with the
 *      neighbouring ranks over RCCL send/recv, reproject the output rows that need only owned rows while the
 *      halo travels, then the rest.  The plan describes this rank's windows: src is its resident buffer
 *      ([nc,] src_nrows, nx) holding the rows it owns -- [own_row0, own_row0 + own_nrows), absolute -- with room
 *      for the halo rows around them; sends/recvs list absolute source rows (one RCCL message per component plane,
 *      straight from/into src: nothing is staged).  rccl_comm is the caller's ncclComm_t (one rank per GPU) or one made
 *      by pxl_comm_init_rank; the RCCL functions are looked up in the RCCL instance already loaded in the process
 *      (PXL_RCCL_LIB names it explicitly), never in a second instance loaded behind the caller's back, so this
 *      library has no link-time RCCL dependency.  The exchange runs on a stream owned by the plan,
 *      ordered after everything queued on `stream` before the call; the function does not synchronise.
 *      With no transfers (one rank) it is build_tables + execute.  No reference counterpart.                    */
typedef struct pxl_halo_xfer {
    int32_t peer;        /* rank in rccl_comm */
    int32_t reserved;
    int64_t row0;        /* first source row of the transfer, 0-based, absolute */
    int64_t nrows;
} pxl_halo_xfer;
int pxl_reproject_sharded_step_f64(pxl_reproject_plan* plan, double* src, double* dst,
                                   int64_t own_row0, int64_t own_nrows,
                                   const pxl_halo_xfer* sends, int nsends, const pxl_halo_xfer* recvs, int nrecvs,
                                   void* rccl_comm, void* stream);
int pxl_reproject_sharded_step_f32(pxl_reproject_plan* plan, float* src, float* dst,
                                   int64_t own_row0, int64_t own_nrows,
                                   const pxl_halo_xfer* sends, int nsends, const pxl_halo_xfer* recvs, int nrecvs,
                                   void* rccl_comm, void* stream);

/* ---- RCCL communicator for hosts that have no RCCL binding of their own (a Julia or C host; torch users pass
 *      ProcessGroupNCCL's communicator instead).  Thin wrappers over ncclGetUniqueId / ncclCommInitRank /
 *      ncclCommDestroy.  One rank calls pxl_comm_unique_id and distributes the PXL_COMM_ID_BYTES bytes to the others by
 *      any means (file, MPI, socket); every rank then calls pxl_comm_init_rank (collective) with its HIP device current.
 *      RCCL is looked up in the instance already loaded in the process, else PXL_RCCL_LIB, else the library loads
 *      librccl.so itself -- and then pxl_reproject_sharded_step_* only accepts communicators created here (a
 *      communicator means nothing to another RCCL instance).  pxl_comm_backend() says which instance is in use.     */
#define PXL_COMM_ID_BYTES 128
int pxl_comm_unique_id(void* id128);
int pxl_comm_init_rank(const void* id128, int rank, int nranks, void** comm);
int pxl_comm_destroy(void* comm);
const char* pxl_comm_backend(void);

/* one-shot convenience (creates a plan, executes, synchronises `stream`, destroys) */
int pxl_reproject_car_bilinear_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* src,
                                   const pxl_car_wcs* wcs_out, const int64_t shape_out[2], double* dst,
                                   void* stream);

/* ---- Generic (non-separable) bilinear reprojection between CAR and Gnomonic maps: per output pixel
 *      pix2sky(out) -> sky2pix(in) -> 2x2 gather, with the evaluators of car_proj.jl / tan_proj.jl.
 *      The coordinate map is interpolated per 128 x 32 output tile (degree 6 x 5 from 42 exact evaluations) and the
 *      interpolant checked against twelve more exact evaluations to 1e-10 pixel; tiles that fail the check (and every tile with
 *      PXL_GENERIC_EXACT=1) evaluate per pixel (~10 FP64 libm calls each).  Full maps only.
 *      proj codes: PXL_PROJ_CAR, PXL_PROJ_TAN.                                                                   */
#define PXL_PROJ_CAR 0
#define PXL_PROJ_TAN 1
int pxl_reproject_generic_bilinear_f64(const pxl_car_wcs* wcs_in, int proj_in, const int64_t shape_in[3],
                                       const double* src, const pxl_car_wcs* wcs_out, int proj_out,
                                       const int64_t shape_out[2], double* dst, void* stream);

/* The same operator with its coordinate lattice kept: what pxl_reproject_plan is to the separable CAR -> CAR path.  Creating
 * the plan evaluates every tile's lattice and check points once (k_generic_lattice) and records which tiles must be evaluated
 * per pixel; executing it is the pixel kernel alone (plus the per-pixel launch only when such tiles exist), on any source map
 * of the plan's input geometry with any number of components.  A mosaic of patches, or many maps onto one patch, pays the
 * transcendental part once per geometry pair.  Same results as the one-shot entry, bit for bit (same kernels, same lattice).
 * create synchronises `stream` (it reads the count of per-pixel tiles back); execute is asynchronous on its stream.
 * 2.8 MB of device memory per 4096 x 4096 output patch (676 B per tile), owned by the plan.                           */
typedef struct pxl_generic_plan pxl_generic_plan;
int pxl_generic_plan_create(const pxl_car_wcs* wcs_in, int proj_in, const int64_t shape_in[2],
                            const pxl_car_wcs* wcs_out, int proj_out, const int64_t shape_out[2],
                            void* stream, pxl_generic_plan** plan);
int pxl_generic_plan_execute(const pxl_generic_plan* plan, int64_t ncomp, const double* src, double* dst, void* stream);
int pxl_generic_plan_tiles(const pxl_generic_plan* plan, int64_t* exact_tiles, int64_t* total_tiles);
int pxl_generic_plan_destroy(pxl_generic_plan* plan);

/* diagnostics: of the 128 x 32 output tiles of the last tiled pxl_reproject_generic_bilinear_f64 call on the current device,
 * how many evaluated the coordinates per pixel (the interpolant failed its 1e-10-pixel check there: the rewind jump of
 * a periodic source, the Gnomonic horizon, very coarse pixels).  Synchronises `stream`.  Each call counts in a counter of its
 * own; its last launch copies the count to one word per device, which this entry reads.  So the pair is exact for a caller
 * that makes its one-shot calls on `stream` alone; with calls in flight on other streams or threads it reports whichever
 * call last reached that copy (and the tile total of the call enqueued last).  The results of the calls never depend on it.
 * Calls with PXL_GENERIC_EXACT=1 or more than 65 535 tile rows (per-pixel kernel only) leave it unchanged.  Plans:
 * pxl_generic_plan_tiles.                                                                                               */
int pxl_reproject_generic_last_tiles(int64_t* exact_tiles, int64_t* total_tiles, void* stream);

/* ---- Scattered bilinear sample: (x, y) = sky2pix!(shape_in, wcs_in, sky2xN; safe=true)
 *      [car_proj.jl:165-193] then the same 2x2 gather + lerp.  out is (n, nc) column-major.          */
int pxl_sample_car_bilinear_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* src,
                                int64_t src_row0, int64_t src_nrows,
                                int64_t n, const double* sky2xN, double* out, void* stream);

int pxl_sample_car_bilinear_f32(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const float* src,
                                int64_t src_row0, int64_t src_nrows,
                                int64_t n, const double* sky2xN, float* out, void* stream);

/* ---- Scatter-add, the transpose of pxl_sample_car_bilinear_f64 (python-pixell's
 *      interpol.map_coordinates(..., trans=True); NOT in the reference).  dst holds rows [row0, row0+nrows) of every
 *      component plane of the (nx, ny, nc) map, (nx, nrows, nc) column-major, with the window meaning of the sampler's
 *      src; vals is (n, nc) column-major like the sampler's out.  For point k the position (x, y), the cell
 *      i0 = floor(x), j0 = floor(y), the fractions fx, fy, the column rule (wrapped on a full-circle map, otherwise on
 *      the map only inside [1, nx]) and the row rule (inside [1, ny] and inside the window) are the sampler's, bit for
 *      bit.  For every component c and each of the four taps (a, b) in {0, 1}^2 that is on the map,
 *          dst[c][j0+b][i0+a] += (wy_b * wx_a) * vals[c][k],   wx = (1-fx, fx), wy = (1-fy, fy),
 *      the product formed in that order without fma.  A tap the sampler reads as 0 is dropped.  A point whose x or y is
 *      not finite contributes NOTHING (the sampler returns NaN there; the transpose has nowhere to put it).  A
 *      non-finite value goes to its four taps by the arithmetic above, zero-weight taps included (0 * NaN = NaN).
 *      dst is accumulated into, not overwritten; pixels that receive no term keep their bits.
 *      NOT REPRODUCIBLE IN THE LAST BITS: the adds are hardware FP64 atomics (global_atomic_add_f64) and the order of
 *      the additions into one pixel is unspecified, so two calls on the same inputs may differ in the last bits wherever
 *      a pixel receives more than one non-zero term (each within (k - 1) * 2^-53 * sum|term| of the exact sum of its k terms, the pixel's initial value counted as one).
 *      Float64 and CAR only.  dst must be ordinary device memory (hipMalloc: hardware FP64 atomics are the path; they
 *      are not defined on fine-grained or host-mapped memory) and may not overlap vals or sky2xN.
 *      PXL_EINVAL before any write: an invalid WCS or shape (nc < 1), a window outside [0, ny], n < 0, a null pointer
 *      with n > 0 (dst may be null only when nrows = 0), sky2xN not 16-byte aligned, dst overlapping vals or sky2xN.
 *      n = 0 or nrows = 0 returns 0 and launches nothing.  Asynchronous on `stream`, no synchronisation, no scratch. */
int pxl_scatter_car_bilinear_f64(const pxl_car_wcs* wcs, const int64_t shape[3], double* dst,
                                 int64_t row0, int64_t nrows, int64_t n, const double* sky2xN,
                                 const double* vals_ncxN, void* stream);

/* ---- The same sample from a ROW-PAIR copy of the map (caller-owned, 64-byte aligned, pxl_sample_pairs_elems() map
 *      elements = 8/3 of the resident window plus one row): an entry holds (v[p-1][i], v[p][i]), and the entries of a
 *      row are stored in 64-byte groups that overlap by one entry (4 Float64 / 8 Float32 entries per group, columns
 *      past nx wrapping round), so a point's whole 2x2 neighbourhood is two adjacent entries of ONE 64-byte sector:
 *      1.0 instead of 2.25 random sectors per point.  The element count covers either element type (a Float32 copy
 *      of a large map uses 6/7 of it).  Build once per map (one streaming pass), sample any number of batches; results are
 *      bit-identical to pxl_sample_car_bilinear_*.  No reference counterpart (the reference has no sampler,
 *      SURVEY 8(a) R1).                                                                                          */
int64_t pxl_sample_pairs_elems(const int64_t shape_in[3], int64_t src_nrows);      /* -1 on invalid arguments */
int pxl_sample_build_pairs_f64(const int64_t shape_in[3], const double* src, int64_t src_nrows, double* pairs,
                               void* stream);
int pxl_sample_build_pairs_f32(const int64_t shape_in[3], const float* src, int64_t src_nrows, float* pairs,
                               void* stream);
int pxl_sample_car_bilinear_pairs_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* pairs,
                                      int64_t src_row0, int64_t src_nrows,
                                      int64_t n, const double* sky2xN, double* out, void* stream);
int pxl_sample_car_bilinear_pairs_f32(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const float* pairs,
                                      int64_t src_row0, int64_t src_nrows,
                                      int64_t n, const double* sky2xN, float* out, void* stream);

/* ---- Cubic B-spline (order 3) interpolation of CAR maps, Float64 (python-pixell's default order).
 *      NOT in the reference.  Two steps: a prefilter turns the map into B-spline coefficients once, then any number of
 *      reprojections or scattered samples evaluate the 4 x 4-tap spline from the coefficients.
 *
 *      prefilter: coeffs (shape and layout of src, every component a plane of its own) is the solution of
 *      (b[i-1,j] + 4 b[i,j] + b[i+1,j]) / 6 = m[i,j] along RA, then of the same system along DEC on b.  Boundary along RA:
 *      cyclic iff nx * |cdelt[0] * unit| is within 1e-8 of 2 pi (the bilinear path's test), otherwise, and always along DEC,
 *      whole-sample mirror (c[0] = c[2], c[n+1] = c[n-1]).  Each axis is one launch: the system factors into a causal and an
 *      anti-causal recursion with the pole sqrt(3) - 2, and a block starts both 32 samples early (|pole|^32 = 5e-19) on the map
 *      extended by the boundary rule, so blocks are independent and the result does not depend on their schedule.
 *      Scratch: one map-sized buffer from the library's stream-ordered pool (pxl_release_scratch).  Asynchronous on `stream`.
 *
 *      evaluation at a source position (x, y): i0 = floor(x), f = x - i0, taps i0-1 .. i0+2 with the weights (1-f)^3/6,
 *      (3f^3 - 6f^2 + 4)/6, (-3f^3 + 3f^2 + 3f + 1)/6, f^3/6, the same in y; the RA sum of each tap row first, each sum left to
 *      right, no fma.  Tap indices outside [1, n] wrap on a periodic RA axis and are mirrored otherwise.  The value is +0.0
 *      where y is outside [0.5, ny + 0.5] and, on a non-periodic map, where x is outside [0.5, nx + 0.5].  (x, y) are the
 *      bilinear entries' positions, bit for bit: the plan's tables for the reprojection (division form), sky2pix!(safe=true)
 *      in the reciprocal form for scattered points.  dst, sky2xN and out are laid out as for the bilinear entries (out is
 *      (n, nc) column-major; a point whose position is not finite gives NaN).  Full maps only.
 *      PXL_EINVAL before any device work: a null pointer, an invalid WCS or shape, nx or ny < 4, coeffs overlapping src
 *      (prefilter), dst overlapping coeffs (reprojection).
 *
 *      Non-finite pixels (NaN, +-Inf), all three entries.  The coefficient at a non-finite pixel is non-finite, so every
 *      reprojected or sampled value whose 4 x 4 support holds that pixel is non-finite -- never a finite number.  The pixel's
 *      influence has a fixed reach: a lane of the prefilter computes 16 consecutive coefficients from the 32 samples before
 *      the first to the 32 after the last, so a coefficient can be non-finite only within 32 + 16 - 1 = 47 columns AND 47 rows
 *      of a non-finite pixel (cyclic distance along a periodic RA axis), an evaluated value only where one of its 4 x 4 taps
 *      is.  Which of the coefficients inside that rectangle are non-finite depends on the pixel's position in the block
 *      layout and is not part of the contract (the exact solution of the system would be non-finite along whole rows and
 *      columns; the difference between any two finite replacements of the pixel decays as 0.268^distance and is below
 *      1e-27 of its size at the edge of the rectangle).  Everything outside the rectangle is what the map with the non-finite
 *      pixels replaced by any finite value gives, within the error bound of DESIGN.md 4.9.  Out-of-domain outputs stay +0.0
 *      whatever the taps they would have folded onto hold.  Two calls give the same NaN positions and the same bits elsewhere.
 *      -0.0, subnormal and huge finite pixels are ordinary data (coefficients of pixels near the Float64 limit may overflow:
 *      an isolated spike's coefficient is 3 x the spike).                                                              */
int pxl_spline_prefilter_car_f64(const pxl_car_wcs* wcs, const int64_t shape[3], const double* src, double* coeffs, void* stream);
int pxl_reproject_car_cubic_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* coeffs,
                                const pxl_car_wcs* wcs_out, const int64_t shape_out[2], double* dst, void* stream);
int pxl_sample_car_cubic_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* coeffs,
                             int64_t n, const double* sky2xN, double* out, void* stream);

/* ---- The transpose of the order-3 sampler (python-pixell's
 *      interpol.map_coordinates(..., order=3, trans=True); NOT in the reference).  The sampler is P = E F, F the prefilter and
 *      E the 4 x 4-tap evaluation of pxl_sample_car_cubic_f64, so P^T = F^T E^T: scatter first, transposed prefilter second,
 *          pxl_scatter_car_cubic_f64(dst = zeros, d);  pxl_spline_prefilter_transpose_car_f64(dst -> result)
 *      gives <P m, d> = <m, P^T d> at rounding level.  The UNtransposed prefilter is the wrong second step: it misses the
 *      identity by 1e-3 .. 1e-2 on every map (DEC is always a mirrored axis).  E^T is linear in d, so any number of batches
 *      may be scattered into one map before F^T is applied once.  Float64 CAR maps, full maps only.
 *
 *      scatter (E^T): dst is the (nx, ny, nc) map, vals is (n, nc) column-major like the sampler's out.  For point k the
 *      position (x, y) = sky2pix!(safe=true) in the reciprocal form, the cell i0 = floor(x), j0 = floor(y), the fractions, the
 *      domain rule (y inside [0.5, ny + 0.5] and, on a non-periodic map, x inside [0.5, nx + 0.5]), the four weights per axis
 *      and the tap indices i0-1 .. i0+2, j0-1 .. j0+2 folded onto the map (wrapped on a periodic RA axis, mirrored otherwise)
 *      are the sampler's, bit for bit.  For every component c and each of the sixteen taps (a, b)
 *          dst[c][row_b][col_a] += (wy[b] * wx[a]) * vals[c][k],
 *      the product formed in that order without fma.  Taps that fold onto the same pixel next to a mirrored edge are each added
 *      on their own.  A point whose x or y is not finite, or which lies outside the domain, contributes NOTHING (the sampler
 *      returns NaN or 0 there).  A non-finite value goes to its sixteen taps by the arithmetic above, zero-weight taps
 *      included (0 * NaN = NaN).  dst is accumulated into, not overwritten; pixels that receive no term keep their bits.
 *      NOT REPRODUCIBLE IN THE LAST BITS: the adds are hardware FP64 atomics (global_atomic_add_f64) and the order of the
 *      additions into one pixel is unspecified, so two calls on the same inputs may differ in the last bits wherever a pixel
 *      receives more than one non-zero term (each within (k - 1) * 2^-53 * sum|term| of the exact sum of its k terms, the
 *      pixel's initial value counted as one).  dst must be ordinary device memory (hipMalloc), as for the bilinear scatter.
 *      PXL_EINVAL before any write: an invalid WCS or shape (nc < 1), nx or ny < 4, n < 0, a null pointer with n > 0,
 *      sky2xN not 16-byte aligned, dst overlapping vals or sky2xN.  n = 0 returns 0 and launches nothing.  Asynchronous on
 *      `stream`, no synchronisation, no scratch.
 *
 *      transposed prefilter (F^T): dst (shape and layout of src) is the solution of the TRANSPOSED systems of
 *      pxl_spline_prefilter_car_f64, along RA, then along DEC.  On a cyclic RA axis the system is symmetric and the pass is the
 *      prefilter's.  On a mirrored axis (DEC always; RA unless the map is full-circle) the system matrix B has B[1,2] =
 *      B[n,n-1] = 2/6 against B[2,1] = B[n-1,n] = 1/6; with D = diag(1/2, 1, .., 1, 1/2) D B is symmetric, so
 *      B^-T = D B^-1 D^-1: the two edge lines of the axis are doubled, the prefilter's recursion runs on that (its warm-up sees
 *      the mirror extension of the doubled input), and the same two lines are halved.  Both scalings are exact; the kernels,
 *      the launches, the scratch (one map-sized buffer from the library's pool) and the block independence are the
 *      prefilter's.  Non-finite pixels have the prefilter's reach: an output can be non-finite only within 47 columns AND 47
 *      rows of a non-finite input pixel, and everything outside that rectangle is what the input with those pixels replaced by
 *      any finite value gives, within the error bound of DESIGN.md 4.11.
 *      PXL_EINVAL before any device work: a null pointer, an invalid WCS or shape, nx or ny < 4, dst overlapping src.
 *      Asynchronous on `stream`.                                                                                          */
int pxl_scatter_car_cubic_f64(const pxl_car_wcs* wcs, const int64_t shape[3], double* dst, int64_t n, const double* sky2xN,
                              const double* vals_ncxN, void* stream);
int pxl_spline_prefilter_transpose_car_f64(const pxl_car_wcs* wcs, const int64_t shape[3], const double* src, double* dst,
                                           void* stream);

/* ---- The polarised pointing matrix: fused IQU sample and scatter-add (NOT in the reference).  A detector
 *      sample of a polarised sky is d = I + q Q + u U with the response q = gamma cos 2 psi, u = gamma sin 2 psi.  The caller
 *      forms (q, u): no trigonometry runs on the device.  The map is a Float64 CAR map of exactly three component planes
 *      I, Q, U (shape[2] = 3); sky2xN is the coordinate batch of the scalar entries; resp2xN is the response batch in the same
 *      layout, interleaved (q_k, u_k) pairs, 16-byte aligned.  Q and U are treated as three independent scalar planes: NO spin-2
 *      sign flip is applied at the DEC mirror or across a pole.
 *
 *      forward (P_pol): out is (n), one value per point.  With s_c[k] what pxl_sample_car_bilinear_f64 (src, window and all)
 *      or pxl_sample_car_cubic_f64 (coeffs) returns for component c at point k, bit for bit,
 *          out[k] = (s_I + q_k * s_Q) + u_k * s_U,
 *      evaluated left to right without fma.  NaN at a position that is not finite, +0.0 terms outside the order-3 domain or on
 *      dropped bilinear taps, NaN and Inf propagation all follow from that formula.
 *
 *      transpose (P_pol^T): vals is (n), one value v per point, and t_0 = v, t_1 = q_k * v, t_2 = u_k * v.  mode 0 (signal): dst
 *      holds the three planes I, Q, U and plane c receives exactly the adds pxl_scatter_car_bilinear_f64 (row window and all) or
 *      pxl_scatter_car_cubic_f64 would make for vals[c][k] = t_c: the term (wy_b * wx_a) * t_c on the same taps, with the same
 *      seam, fold, domain, window and live rules, zero-weight taps included, by the same no-return agent-scope FP64 atomic under
 *      the same clause on the last bits.  mode 1 (weights): dst holds SIX planes II, IQ, IU, QQ, QU, UU, v is the sample
 *      weight and t_3 = q_k * t_1, t_4 = q_k * t_2, t_5 = u_k * t_2: P^T applied to the six products, the block
 *      preconditioner and hit map of a polarised map-maker.  shape[2] stays 3 in both modes (it describes the IQU map).
 *      The cubic entries are the evaluation E and its transpose E^T only, on full maps: compose them with
 *      pxl_spline_prefilter_car_f64 and pxl_spline_prefilter_transpose_car_f64 as the scalar entries are.
 *
 *      PXL_EINVAL before any write: whatever the scalar counterpart refuses, shape[2] != 3, mode other than 0 or 1, resp2xN
 *      null with n > 0 or not 16-byte aligned, dst overlapping sky2xN, resp2xN or vals.  n = 0 (or nrows = 0) returns 0 and
 *      launches nothing.  Asynchronous on `stream`, no synchronisation, no scratch.                                          */
int pxl_sample_car_pol_bilinear_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* src,
                                    int64_t src_row0, int64_t src_nrows, int64_t n, const double* sky2xN,
                                    const double* resp2xN, double* out, void* stream);
int pxl_sample_car_pol_cubic_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* coeffs, int64_t n,
                                 const double* sky2xN, const double* resp2xN, double* out, void* stream);
int pxl_scatter_car_pol_bilinear_f64(const pxl_car_wcs* wcs, const int64_t shape[3], double* dst, int64_t row0,
                                     int64_t nrows, int64_t n, const double* sky2xN, const double* resp2xN,
                                     const double* vals, int mode, void* stream);
int pxl_scatter_car_pol_cubic_f64(const pxl_car_wcs* wcs, const int64_t shape[3], double* dst, int64_t n,
                                  const double* sky2xN, const double* resp2xN, const double* vals, int mode, void* stream);

/* ---- The per-pixel IQU block solve and block product (NOT in the reference): what turns P^T W d and the six
 *      weight planes of the mode-1 scatters above into a map.  weights6 holds the six planes II, IQ, IU, QQ, QU, UU of npix
 *      pixels each, contiguous with stride npix; rhs3 / x3 / out3 hold three planes I, Q, U the same way; rcond holds one plane,
 *      or is null.  Per pixel a, b, c, d, e, f are the six weights, A = [a b c; b d e; c e f], and r0, r1, r2 the right-hand
 *      side.  All Float64; every operation below is ONE IEEE rounding, no fma, no transcendental, so the result is defined to
 *      the bit (tests/polsolve_ref.py restates it in numpy).  The method is LDL^T with diagonal pivoting, rank-revealing on the
 *      positive semi-definite blocks a pointing matrix produces:
 *
 *        first pivot    i1 = (a >= d && a >= f) ? 0 : (d >= f ? 1 : 2); rows and columns permuted to (0,1,2), (1,0,2) or (2,0,1)
 *                       (i1 first, the other two in order); m11, m21, m31, m22, m32, m33 the permuted entries, R1, R2, R3 the
 *                       permuted right-hand side
 *        elimination    p1 = m11, l21 = m21 / p1, l31 = m31 / p1,
 *                       s22 = m22 - l21 * m21, s33 = m33 - l31 * m31, s32 = m32 - l31 * m21
 *        second pivot   if s33 > s22: exchange s22 and s33, l21 and l31, R2 and R3, and the last two of the permutation
 *        elimination    p2 = s22, l32 = s32 / p2, p3 = s33 - l32 * s32
 *        conditioning   rc2 = p2 / p1, rc3 = p3 / p1, rc = (rc3 < rc2) ? rc3 : rc2, fin = r0, r1 and r2 are all finite
 *                       ok  = fin && p1 > 0 && rc2 >= rcond_min && rc3 >= rcond_min
 *                       rcond plane = (fin && p1 > 0 && rc2 > 0 && rc3 > 0) ? rc : +0.0
 *        solve          y1 = R1, y2 = R2 - l21 * y1, y3 = (R3 - l31 * y1) - l32 * y2,
 *                       x3 = y3 / p3, x2 = y2 / p2 - l32 * x3, x1 = (y1 / p1 - l21 * x2) - l31 * x3, un-permuted into out3;
 *                       where ok is false all three outputs are +0.0
 *
 *      Every comparison is false on NaN, so a NaN or an infinity in any weight, or in the right-hand side (fin), gives "not
 *      solved, rcond +0.0"; so do the zero block, a largest diagonal entry <= 0 and every block of rank below 3 (a pixel hit
 *      fewer than three times, or at one polarisation angle).  rc lies between lambda_min / lambda_max of the block and a small
 *      multiple of it (p3 >= lambda_min, p1 <= lambda_max).
 *
 *      apply is the block product: out = A x, y0 = (a * x0 + b * x1) + c * x2, y1 = (b * x0 + d * x1) + e * x2,
 *      y2 = (c * x0 + e * x1) + f * x2, left to right.
 *
 *      out3 may be exactly rhs3 / x3 (in place).  PXL_EINVAL before any write: a null weights6, rhs3 / x3 or out3 with npix > 0,
 *      npix < 0, npix > INT64_MAX / 48 (the byte sizes would overflow), a pointer not 8-byte aligned, rcond_min not finite or outside (0, 1], out3 overlapping weights6 or rcond, out3
 *      overlapping rhs3 / x3 other than exactly, rcond overlapping any input.  npix = 0 returns 0 and launches nothing.
 *      Asynchronous on `stream`, no synchronisation, no scratch.                                                              */
int pxl_pol_block_solve_f64(const double* weights6, const double* rhs3, double* out3, double* rcond, int64_t npix,
                            double rcond_min, void* stream);
int pxl_pol_block_apply_f64(const double* weights6, const double* x3, double* out3, int64_t npix, void* stream);

/* ---- The normal operator of the polarised map-maker: y += P^T W P x in one pass (NOT in the reference).  P is
 *      the order-1 pointing matrix above (pxl_sample_car_pol_bilinear_f64), W = diag(w) the sample weights.  x3 and y3 are
 *      Float64 CAR maps of exactly three planes I, Q, U (shape[2] = 3), FULL MAPS ONLY: there is no row window here (a
 *      declination strip goes through the two entries above).  sky2xN and resp2xN are the batches of those entries, w is (n).
 *      Per point k, in this order: the position, cell, fractions and four tap offsets of the bilinear entries, formed once;
 *      the twelve taps of x3; s_c = (1-fy) * ((1-fx) * m00 + fx * m10) + fy * ((1-fx) * m01 + fx * m11) per plane, a dropped
 *      tap read as 0; d = (s_0 + q_k * s_1) + u_k * s_2; v = w[k] * d, one rounding; then exactly the adds
 *      pxl_scatter_car_pol_bilinear_f64 (mode 0, the whole map) makes for the value v: (wy_b * wx_a) * t_c with
 *      t = (v, q_k * v, u_k * v) on every tap that is on the map, zero weights included.  No fma anywhere.
 *      THE CONTRACT: the call adds to y3 the same multiset of terms, bit for bit, as
 *          pxl_sample_car_pol_bilinear_f64 into a temporary d, v[k] = w[k] * d[k], pxl_scatter_car_pol_bilinear_f64 of v into y3
 *      would; only the order of the atomic adds into one pixel is unspecified, under the clause the scatters carry: NOT
 *      REPRODUCIBLE IN THE LAST BITS wherever a pixel receives more than one non-zero term (each result within
 *      (k - 1) * 2^-53 * sum|term| of the exact sum of its k terms, the pixel's initial value counted as one).  A point whose
 *      position is not finite adds NOTHING: the sampler's NaN for it never reaches the map.  A non-finite pixel of x3 or a
 *      non-finite w[k] therefore makes the four taps of every point that reads it NaN in all three planes (0 * NaN = NaN),
 *      as the composition does.  y3 is accumulated into, not overwritten; pixels that receive no term keep their bits.  x3 is
 *      only read, y3 only written, and only through the atomics; y3 must be ordinary device memory, as for the scatters.
 *      PXL_EINVAL before any write: an invalid WCS or shape, shape[2] != 3, n < 0, a null x3, y3, sky2xN, resp2xN or w with
 *      n > 0, sky2xN or resp2xN not 16-byte aligned, sizes whose byte counts overflow, y3 overlapping x3, sky2xN, resp2xN or
 *      w.  n = 0 returns 0 and launches nothing.  Asynchronous on `stream`, no synchronisation, no scratch.               */
int pxl_normal_car_pol_bilinear_f64(const pxl_car_wcs* wcs, const int64_t shape[3], const double* x3, double* y3, int64_t n,
                                    const double* sky2xN, const double* resp2xN, const double* w, void* stream);

/* ---- Nearest-pixel (order 0) pointing and the one-pass binned IQU accumulation (NOT in the reference).
 *      Float64 and CAR only.  Arguments, layouts and row windows are those of the bilinear counterparts above
 *      (pxl_sample_car_bilinear_f64, pxl_scatter_car_bilinear_f64, pxl_sample_car_pol_bilinear_f64,
 *      pxl_scatter_car_pol_bilinear_f64).
 *
 *      THE PIXEL of point k: (x, y) is the position the bilinear entries form, bit for bit (sky2pix!, safe = true).  With
 *      i0 = floor(x), fx = x - i0 (exact), j0 = floor(y), fy = y - j0 (exact; i0 and j0 clamped to +-2^30 as there),
 *          i = i0 + (fx >= 0.5),   j = j0 + (fy >= 0.5):
 *      pixel i owns [i - 0.5, i + 0.5), a tie goes to the HIGHER index, and the rule has no rounding of its own (it is not
 *      floor(x + 0.5), which rounds the sum first).  Column: on a full-circle map i is wrapped into [1, nx] (x = nx + 0.5 is
 *      column 1), otherwise the point is on the map iff 1 <= i <= nx.  Row: on the map iff 1 <= j <= ny (y = 0.5 is row 1,
 *      y = ny + 0.5 is off the map) and row j - 1 lies inside the window [row0, row0 + nrows).
 *
 *      sample: out[c][k] is that pixel's value of plane c UNCHANGED -- no arithmetic, so -0.0, subnormals, +-Inf and NaN come
 *      back as bits; +0.0 for a point that is not on the map; NaN where x or y is not finite.  sample_pol:
 *      out[k] = (s_I + q_k * s_Q) + u_k * s_U of those per-plane values, left to right without fma.
 *
 *      scatter: dst[c][pixel] += vals[c][k], the value itself with no product, by ONE no-return agent-scope FP64 atomic per
 *      plane; a point that is not on the map, or whose x or y is not finite, adds NOTHING.  scatter_pol: plane c takes t_c
 *      with t_0 = v, t_1 = q_k * v, t_2 = u_k * v (mode 0, three planes I Q U) and t_3 = q_k * t_1, t_4 = q_k * t_2,
 *      t_5 = u_k * t_2 (mode 1, six planes II IQ IU QQ QU UU, v the sample weight), each product one rounding; shape[2] stays 3.
 *      A non-finite value reaches exactly its one pixel per plane.
 *
 *      bin_pol: the fused map-making pass over (d, w, sky2xN, resp2xN), FULL MAPS ONLY (no row window).  Per point
 *      v = w[k] * d[k] with one rounding; rhs3 (three planes) takes the mode-0 terms of v and weights6 (six planes) the mode-1
 *      terms of w[k]: nine adds.  THE CONTRACT: the same multiset of terms, bit for bit, as pxl_scatter_car_pol_nearest_f64
 *      (mode 0) of the products w[k] * d[k] into rhs3 plus pxl_scatter_car_pol_nearest_f64 (mode 1) of w into weights6.
 *      Because a point touches one pixel, weights6 is then EXACTLY P^T W P (it has no other entries) and
 *      pxl_pol_block_solve_f64(weights6, rhs3) is the least-squares map for this P.
 *
 *      All maps written are accumulated into, not overwritten; pixels that receive no term keep their bits.  NOT
 *      REPRODUCIBLE IN THE LAST BITS: the order of the atomic additions into one pixel is unspecified, so two calls on the
 *      same inputs may differ in the last bits wherever a pixel receives more than one non-zero term (each result within
 *      (k - 1) * 2^-53 * sum|term| of the exact sum of its k terms, the pixel's initial value counted as one).  Maps written
 *      must be ordinary device memory, as for the bilinear scatters.
 *      PXL_EINVAL before any write: whatever the bilinear counterpart refuses (an invalid WCS or shape, a window outside
 *      [0, ny], n < 0, a null pointer with n > 0, a 2xN batch not 16-byte aligned, shape[2] != 3 or a bad mode for the
 *      polarised entries, sizes whose byte counts overflow, a map written overlapping an input); for bin_pol also rhs3
 *      overlapping weights6, or either overlapping sky2xN, resp2xN, d or w.  n = 0 (or nrows = 0) returns 0 and writes
 *      nothing.  Asynchronous on `stream`, no synchronisation, no scratch.                                                  */
int pxl_sample_car_nearest_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* src,
                               int64_t src_row0, int64_t src_nrows, int64_t n, const double* sky2xN, double* out,
                               void* stream);
int pxl_scatter_car_nearest_f64(const pxl_car_wcs* wcs, const int64_t shape[3], double* dst, int64_t row0, int64_t nrows,
                                int64_t n, const double* sky2xN, const double* vals_ncxN, void* stream);
int pxl_sample_car_pol_nearest_f64(const pxl_car_wcs* wcs_in, const int64_t shape_in[3], const double* src,
                                   int64_t src_row0, int64_t src_nrows, int64_t n, const double* sky2xN,
                                   const double* resp2xN, double* out, void* stream);
int pxl_scatter_car_pol_nearest_f64(const pxl_car_wcs* wcs, const int64_t shape[3], double* dst, int64_t row0,
                                    int64_t nrows, int64_t n, const double* sky2xN, const double* resp2xN,
                                    const double* vals, int mode, void* stream);
int pxl_bin_car_pol_nearest_f64(const pxl_car_wcs* wcs, const int64_t shape[3], double* rhs3, double* weights6, int64_t n,
                                const double* sky2xN, const double* resp2xN, const double* d, const double* w,
                                void* stream);

/* ---- The two passes of the destriping map-maker (NOT in the reference): the model d = P m + F a + n with P the
 *      nearest-pixel polarised pointing matrix above, n white noise of weights w, and F spreading one amplitude over each
 *      BASELINE, baseline_len consecutive samples of one detector.  Float64, CAR, full maps only.
 *
 *      THE LAYOUT.  An observation is (D, T) with n_base = ceil(T / baseline_len) baselines per detector (the last may be
 *      short); the amplitudes are a vector of n_det * n_base doubles, baseline b = det * n_base + t / baseline_len.  Both entries
 *      work on ONE TIME CHUNK as pxl_pointing_expand_f64 writes it: times [t0, t0 + n_chunk) of all n_det detectors,
 *      detector-major, N = n_det * n_chunk samples; sample k has det = k / n_chunk, j = k % n_chunk and baseline
 *      b = det * n_base + (t0 + j) / baseline_len.  sky2xN, resp2xN, w and d hold N samples in that order.
 *
 *      THE SAMPLE VALUE, one definition for both:  x_k = d[k] (a null),  x_k = a[b] (d null),  x_k = d[k] - a[b] with one
 *      rounding (both given).  THE CUT RULE, one definition for both: sample k is CUT, and contributes nothing anywhere, when
 *      its position is not finite, when it is not on the map (THE PIXEL rule of the nearest-pixel entries, no row window), or
 *      when mask[pixel] is not > 0 (NaN included); mask is one (ny, nx) plane, null = keep everything.  What d, a or w hold
 *      at a cut sample does not matter: a NaN there reaches nothing.
 *
 *      bin:  rhs3 += P^T (w o x) over the uncut samples.  v = w[k] * x_k with one rounding, then the three mode-0 terms of
 *      pxl_scatter_car_pol_nearest_f64 for v, by the same atomics.  THE CONTRACT is bin_pol's: the same multiset of terms, bit
 *      for bit, as pxl_scatter_car_pol_nearest_f64 (mode 0) of the products w[k] * x_k restricted to the uncut samples; rhs3 is
 *      accumulated into, pixels that receive no term keep their bits, and the last-bits clause of the scatters applies (NOT
 *      REPRODUCIBLE IN THE LAST BITS: each pixel within (k - 1) * 2^-53 * sum|term| of the exact sum of its k terms).  rhs3
 *      must be ordinary device memory, as for bin_pol.
 *
 *      project:  out[b] += sum over the uncut samples k of baseline b in this chunk of  w[k] * (x_k - s_k),
 *      s_k = (s_I + q_k * s_Q) + u_k * s_U of map3 at the sample's pixel, pxl_sample_car_pol_nearest_f64's operations in its
 *      order: two roundings per term.  With map3 null the subtraction is skipped and the term is w[k] * x_k, one rounding.
 *      NO ATOMICS: each (baseline, chunk) segment is summed by one owner in an order fixed by the arguments -- lanes stride
 *      through the segment, a fixed tree joins the lane sums -- and added to out[b] by one plain load, add and store.  Two
 *      calls on the same arguments give the same bits; a segment's sum of n terms is within n * 2^-52 * sum|term| of exact.
 *      A baseline that spans chunks is accumulated chunk by chunk; a baseline none of whose samples in this chunk is uncut
 *      keeps its bits, as do all baselines outside the chunk.  out holds n_det * n_base doubles.
 *
 *      PXL_EINVAL before any write: whatever pxl_bin_car_pol_nearest_f64 refuses (an invalid WCS or shape, shape[2] != 3, a
 *      null sky2xN, resp2xN, w, rhs3 or out with N > 0, a 2xN batch not 16-byte aligned); d and a both null; n_det, n_chunk,
 *      t0 or n_base negative; baseline_len < 1; n_chunk > 0 and (t0 + n_chunk - 1) / baseline_len >= n_base; t0 + n_chunk,
 *      n_det * n_chunk, n_det * n_base or a byte count overflowing int64_t; rhs3 or out overlapping sky2xN, resp2xN, w, d, a,
 *      mask or map3.  mask may be null in both, map3 only in project.  N = 0 returns 0 and writes nothing.  Asynchronous
 *      on `stream`, no synchronisation, no scratch.                                                                        */
int pxl_baseline_bin_car_pol_nearest_f64(const pxl_car_wcs* wcs, const int64_t shape[3], double* rhs3, const double* mask,
                                         int64_t n_det, int64_t n_chunk, int64_t t0, int64_t baseline_len, int64_t n_base,
                                         const double* sky2xN, const double* resp2xN, const double* w, const double* d,
                                         const double* a, void* stream);
int pxl_baseline_project_car_pol_nearest_f64(const pxl_car_wcs* wcs, const int64_t shape[3], const double* map3,
                                             const double* mask, int64_t n_det, int64_t n_chunk, int64_t t0,
                                             int64_t baseline_len, int64_t n_base, const double* sky2xN, const double* resp2xN,
                                             const double* w, const double* d, const double* a, double* out, void* stream);

/* ---- The per-scan polynomial filter of a timestream (NOT in the reference): the projection
 *      Z = I - F (F^T W_f F)^-1 F^T W_f, F the Legendre basis of every (detector, segment), applied to d.  Float64.
 *
 *      THE LAYOUT.  d, wfit and out are (n_det, n_t) row-major.  seg_start is a DEVICE array of n_seg + 1 sample offsets shared
 *      by all detectors; segment s is the times [seg_start[s], seg_start[s+1]) of each detector after both ends are clamped to
 *      [0, n_t], empty where the clamped end is not above the start.  The call is memory-safe for any contents of seg_start;
 *      where it is not non-decreasing, segments overlap and the values of out in the overlaps are unspecified.  Samples in no
 *      segment (before seg_start[0], from seg_start[n_seg] on) are copied, out = d bit for bit.  wfit null is the weight 1.0
 *      everywhere, bit for bit the same as an array of ones.  coeffs, (n_det, n_seg, order + 1), and n_used, (n_det, n_seg), may
 *      be null; an empty segment has n_used = 0.
 *
 *      THE DEFINITION, every operation rounded once, none fused.  Sample j of a segment of L samples has
 *      x_j = double((2j + 1) - L) / double(L);  P_0 = 1, P_1 = x, P_(n+1) = ((double(2n+1) * x) * P_n - double(n) * P_(n-1)) /
 *      double(n+1).  A sample is LIVE when wfit > 0 (NaN is not); one that is not contributes nothing to the fit and its d is
 *      not read into any sum: a NaN there stays local.  Over the live samples G_ik = sum (w * P_i) * P_k for i >= k and
 *      b_i = sum (w * P_i) * d.  NO ATOMICS: one group of G lanes owns a (detector, segment); lane l sums the terms of samples
 *      l, l + G, ... in that order from +0.0, and a fixed tree joins the lane sums (v_l + v_(l ^ G/2), ..., v_l + v_(l ^ 1)
 *      within a wavefront; for G = 256 the four wavefronts as (s0 + s1) + (s2 + s3)).  G is a power of two, 1 to 64, or 256,
 *      chosen from n_t, n_seg and order alone: 256 where n_t / max(n_seg, 1) >= 1024 (integer division), else the smallest
 *      power of two >= ceil((n_t / max(n_seg, 1)) / (order + 1)), at most 64.  Two calls on the same arguments give the same
 *      bits.  The solve is LDL^T of G without pivoting in the Legendre order: U_ik = G_ik - sum_(m<k) U_im * L_km (m ascending),
 *      L_ik = U_ik / D_k, D_i = G_ii - sum_(k<i) U_ik * L_ik (k ascending).  Pivot i is accepted when D_i > rcond_min * G_ii (a NaN
 *      fails) -- relative to G_ii because the last pivots of a segment with fewer live samples than coefficients are rounding
 *      noise, not zeros.  The fit is truncated at the first rejected pivot: n_used is the number of accepted leading pivots,
 *      0 to order + 1; the coefficients from n_used on are exactly +0.0 and the accepted ones solve the leading n_used x n_used
 *      system by the leading part of the same factorisation: y_i = b_i - sum_(m<i) L_im * y_m (m ascending), then from
 *      i = n_used - 1 down c_i = y_i / D_i - sum_(i<m<n_used) L_mi * c_m (m ascending).  The second pass, over every sample of
 *      the segment live or not:  out_j = d_j - f,  f = c_0, f = f + c_n * P_n for n = 1 .. order in order.  With n_used = 0
 *      out_j = d_j bit for bit.  out == d exactly (in place) is allowed.
 *
 *      PXL_EINVAL before any write: order outside 0 .. 7; rcond_min not in [0, 1) or NaN; n_det, n_t or n_seg negative;
 *      n_det * n_t, n_det * n_seg or a byte count overflowing int64_t; with n_det * n_t > 0 a null d, out or seg_start, a
 *      buffer not 8-byte aligned, out overlapping d other than exactly, out, coeffs or n_used overlapping d, wfit, seg_start or
 *      each other, n_det * (n_seg + 2) groups beyond one launch.  n_det * n_t = 0 returns 0 and writes nothing.
 *      Asynchronous on `stream`, no synchronisation, no scratch.                                                           */
int pxl_tod_polyfilter_f64(int64_t n_det, int64_t n_t, int64_t n_seg, const int64_t* seg_start, int order, double rcond_min,
                           const double* d, const double* wfit, double* out, double* coeffs, int64_t* n_used, void* stream);

/* ---- The detector-mode filter of a timestream (NOT in the reference): the polynomial filter's projection
 *      Z = I - F (F^T W_f F)^-1 F^T W_f transposed -- F the caller's (n_det, n_modes) detector couplings, applied across the
 *      detectors of a group, once per time sample.  n_modes = 1 with F = 1 or the gains is the common mode; F = (1, x, y) a plane
 *      across the focal plane; F = eigenvectors a PCA filter.  Float64.
 *
 *      THE LAYOUT.  d, wfit and out are (n_det, n_t) row-major; modes is (n_det, n_modes) row-major, on the DEVICE.  grp_start is
 *      a DEVICE array of n_grp + 1 detector offsets; group g is the detectors [grp_start[g], grp_start[g+1]) after both ends are
 *      clamped to [0, n_det], empty where the clamped end is not above the start.  The call is memory-safe for any contents of
 *      grp_start; where it is not non-decreasing, groups overlap and the values of out in the overlaps are unspecified.
 *      Detectors in no group (before grp_start[0], from grp_start[n_grp] on) are copied, out = d bit for bit.  wfit null is the
 *      weight 1.0 everywhere, bit for bit the same as an array of ones.  amps, (n_grp, n_modes, n_t), and n_used, (n_grp, n_t),
 *      may be null; an empty group has n_used = 0.
 *
 *      THE DEFINITION, every operation rounded once, none fused.  Detector r at time t is LIVE when wfit[r,t] > 0 (NaN is not);
 *      one that is not contributes nothing to the fit and its d is not read into any sum: a NaN there stays local.  Over the
 *      live detectors of the group, w = wfit[r,t]:  G_ik = sum (w * F_ri) * F_rk for i >= k and b_i = sum (w * F_ri) * d[r,t].
 *      NO ATOMICS: a block of 256 lanes owns a (group, tile of C consecutive time samples); its R = 256 / C row phases split the
 *      group's detectors, phase p summing the terms of detectors lo + p, lo + p + R, ... in that order from +0.0, and the
 *      phases are joined by the polynomial filter's tree, v_p = v_p + v_(p ^ off) for off = R/2, ..., 1.  C is 64 where
 *      n_grp * ceil(n_t / 64) >= 512 (the wide tile alone makes two blocks per compute unit), else 16: from n_t and n_grp alone.
 *      Two calls on the same arguments give the same bits.  The solve, the pivot rule and the truncation are
 *      pxl_tod_polyfilter_f64's above, word for word, in the caller's mode order: pivot i is accepted when
 *      D_i > rcond_min * G_ii (a NaN fails), the fit is truncated at the first rejected pivot, n_used (0 to n_modes) is the number
 *      of accepted leading pivots and the amplitudes from n_used on are exactly +0.0.  The second pass, over every detector of
 *      the group live or not:  f = c_0 * F_r0, f = f + c_k * F_rk for k = 1 .. n_modes - 1 in order, out[r,t] = d[r,t] - f.  With
 *      n_used = 0 out = d bit for bit.  out == d exactly (in place) is allowed.
 *
 *      PXL_EINVAL before any write: n_modes outside 1 .. 8; rcond_min not in [0, 1) or NaN; n_det, n_t or n_grp negative;
 *      n_det * n_t, n_det * n_modes, n_grp * n_t * n_modes or a byte count overflowing int64_t; with n_det * n_t > 0 a null d,
 *      out, grp_start or modes, a buffer not 8-byte aligned, out overlapping d other than exactly, out, amps or n_used
 *      overlapping d, wfit, grp_start, modes or each other, (n_grp + 2) * ceil(n_t / C) blocks beyond 2^31 - 1.
 *      n_det * n_t = 0 returns 0 and writes nothing.  Asynchronous on `stream`, no synchronisation, no scratch.               */
int pxl_tod_modefilter_f64(int64_t n_det, int64_t n_t, int64_t n_grp, const int64_t* grp_start, int n_modes, const double* modes,
                           double rcond_min, const double* d, const double* wfit, double* out, double* amps, int64_t* n_used,
                           void* stream);

/* ---- The binned-template filter of a timestream (NOT in the reference): the same projection
 *      Z = I - F (F^T W_f F)^-1 F^T W_f with F the indicator of every (detector, bin) of a plan that sorts the time samples into
 *      bins -- of azimuth, of a half-wave plate's angle, of scan phase and direction: the weighted mean of a bin's live samples
 *      is subtracted from all of its samples, which removes a signal that is a function of the bin alone.  Float64.
 *
 *      THE LAYOUT.  d, wfit and out are (n_det, n_t) row-major.  The plan is shared by all detectors, two DEVICE arrays: order,
 *      n_t sample indices, and bin_start, n_bin + 1 offsets into order.  Bin b of detector r is the samples t = order[j] of row r
 *      for the positions j in [bin_start[b], bin_start[b+1]), both ends clamped to [0, n_t], empty where the clamped end is not
 *      above the start.  The positions in no bin (before bin_start[0], from bin_start[n_bin] on) are copied, out = d bit for bit
 *      at their samples.  A valid plan has order a permutation of 0 .. n_t - 1 and bin_start non-decreasing; then every sample
 *      belongs to one item.  The call is memory-safe for any contents of both: a position with order[j] outside [0, n_t) is
 *      skipped in both passes, its sample neither read nor written; offsets are clamped; where order repeats a sample or the
 *      offsets decrease, the values of out at the samples concerned are unspecified (and a sample that order leaves out is not
 *      written).  wfit null is the weight 1.0 everywhere, bit for bit the same as an array of ones.  means and n_used, both
 *      (n_det, n_bin), may be null.
 *
 *      THE DEFINITION, every operation rounded once, none fused: pxl_tod_polyfilter_f64's above at order 0 with the positions of
 *      a bin in place of the samples of a segment.  A sample is LIVE when wfit > 0 (NaN is not); one that is not contributes
 *      nothing to the fit and its d is not read into any sum: a NaN there stays local.  Over the live positions of the bin
 *      G_00 = sum (w * 1.0) * 1.0 and b_0 = sum (w * 1.0) * d: the bits of sum w and sum w * d.  NO ATOMICS: one group of G lanes
 *      owns a (detector, bin); lane l sums the terms of positions lo + l, lo + l + G, ... in that order from +0.0, and a fixed
 *      tree joins the lane sums (v_l + v_(l ^ G/2), ..., v_l + v_(l ^ 1) within a wavefront; for G = 256 the four wavefronts as
 *      (s0 + s1) + (s2 + s3)).  G is the polynomial filter's at order 0, from n_t and n_bin alone: 256 where
 *      n_t / max(n_bin, 1) >= 1024 (integer division), else the smallest power of two >= n_t / max(n_bin, 1), at most 64.  Two
 *      calls on the same arguments give the same bits.  The mean c = b_0 / G_00 is accepted when G_00 > 0 * G_00, that is for a
 *      positive, finite sum of weights (an infinite one makes 0 * G_00 a NaN, which fails): n_used = 1.  Otherwise n_used = 0, the
 *      mean is exactly +0.0 and the bin is copied, out = d bit for bit.  The second pass, over every position of the bin live
 *      or not:  out = d - c * 1.0.  out == d exactly (in place) is allowed: every first-pass read of an item precedes its first
 *      write.
 *
 *      PXL_EINVAL before any write: n_det, n_t or n_bin negative; n_det * n_t, n_det * n_bin or a byte count overflowing int64_t;
 *      with n_det * n_t > 0 a null d, out, bin_start or order, a buffer not 8-byte aligned, out overlapping d other than exactly,
 *      out, means or n_used overlapping d, wfit, bin_start, order or each other, n_det * (n_bin + 2) groups beyond one launch.
 *      n_det * n_t = 0 returns 0 and writes nothing.  Asynchronous on `stream`, no synchronisation, no scratch.            */
int pxl_tod_binfilter_f64(int64_t n_det, int64_t n_t, int64_t n_bin, const int64_t* bin_start, const int64_t* order, const double* d,
                          const double* wfit, double* out, double* means, int64_t* n_used, void* stream);

/* ---- The banded-Toeplitz noise weight of a timestream (NOT in the reference): out = G T G x, the time-domain
 *      inverse covariance N^-1 of a stationary correlated noise process applied to x -- T one symmetric banded Toeplitz block per
 *      (detector, segment), G the diagonal that zeroes the cut samples ("gappy Toeplitz").  The operator of a maximum-likelihood
 *      map-maker, (P^T N^-1 P) m = P^T N^-1 d.  Float64.
 *
 *      THE LAYOUT.  x, wlive and out are (n_det, n_t) row-major.  kern is (n_det, lambda + 1) row-major on the DEVICE:
 *      kern[r][k] = c_k, the k-th off-diagonal of detector r's blocks.  seg_start is the polynomial filter's: a DEVICE array of
 *      n_seg + 1 sample offsets shared by all detectors; segment s is the times [seg_start[s], seg_start[s+1]) after both ends are
 *      clamped to [0, n_t], empty where the clamped end is not above the start.  The call is memory-safe for any contents of
 *      seg_start, and every segment is found whatever their order; where segments overlap, out is unspecified in the overlaps.
 *      wlive null means every sample is live.
 *
 *      THE DEFINITION, every operation rounded once, none fused.  A sample is LIVE when it lies in a segment and wlive > 0 (NaN
 *      is not).  z_j = x_j where j is live; otherwise z_j = +0.0 and x_j is not read into any sum: a NaN under a cut stays out.
 *      Outside the segment of the output at hand z is +0.0: the blocks do not couple segments.  For a live sample t
 *          S = c_0 * z_t,    then for k = 1 .. lambda in that order    S = S + c_k * (z_(t-k) + z_(t+k)),    out_t = S.
 *      A sample that is not live, or lies in no segment, gets out = +0.0 exactly: this is a weight, and a cut sample weighs
 *      nothing (the filters above copy theirs).  The order of the sum belongs to the output, not to a tiling, so the bits are
 *      fixed by the arguments and two calls give the same bits.  A non-finite live x reaches at most the live samples within
 *      lambda of it inside its segment and nothing else.  No atomics, no scratch, asynchronous on `stream`.
 *
 *      PXL_EINVAL before any write, with a text that starts "tod_toeplitz" and names the argument: lambda outside 0 .. 4096;
 *      n_det, n_t or n_seg negative; n_det * n_t, n_det * (lambda + 1) or a byte count overflowing int64_t; with n_det * n_t > 0
 *      a null x, out, kern or seg_start, a buffer not 8-byte aligned, out overlapping x at all (an output reads its neighbours:
 *      there is no in-place form), out overlapping kern, wlive or seg_start, n_det * ceil(n_t / 1280) blocks beyond 2^31 - 1.
 *      n_det * n_t = 0 returns 0 and writes nothing.                                                                          */
int pxl_tod_toeplitz_f64(int64_t n_det, int64_t n_t, int64_t n_seg, const int64_t* seg_start, int64_t lambda, const double* kern,
                         const double* x, const double* wlive, double* out, void* stream);

/* ---- The gappy autocovariance of a timestream (NOT in the reference): per detector the sums of z_t z_(t+k) over
 *      the pairs of live samples of one segment, k = 0 .. lambda, and the number of those pairs -- the noise estimate from which
 *      the spectrum, and with it kern of pxl_tod_toeplitz_f64 above, is made.  Float64.
 *
 *      THE LAYOUT.  x and wlive are (n_det, n_t) row-major.  seg_start is the Toeplitz weight's: a DEVICE array of n_seg + 1
 *      sample offsets shared by all detectors, segment s the times [seg_start[s], seg_start[s+1]) after both ends are clamped to
 *      [0, n_t], empty where the clamped end is not above the start.  The call is memory-safe for any contents of seg_start and
 *      every segment is found whatever their order; where segments overlap the result is unspecified (inside the buffers).
 *      sums is (n_det, lambda + 1) Float64 and pairs (n_det, lambda + 1) int64_t, or null; both are OVERWRITTEN, every element.
 *
 *      THE DEFINITION, every operation rounded once, none fused.  A sample is LIVE when it lies in a segment and wlive > 0 (NaN is
 *      not; wlive null: every sample of a segment).  z_j = x_j where j is live; otherwise z_j = +0.0 and x_j is not read into any
 *      arithmetic: a NaN under a cut stays out.  For detector r and lag k
 *          sums[r][k] = sum of z_t * z_(t+k) over the t with t and t + k live in the SAME segment,   pairs[r][k] = their number,
 *      exact; a lag with no pair gets +0.0 and 0.  The segments are not coupled.
 *
 *      THE ORDER, from lambda, n_t and the contents of seg_start alone -- not from n_det, the row or the device: a row computed
 *      alone has the bits it has in any larger call, and two calls give the same bits.  need = ceil((lambda + 1) / 5), LPG = the
 *      smallest power of two >= need, at most 256, W = 5 LPG, P = 256 / LPG.  A segment [lo, hi) is walked in tiles of 1280
 *      samples from lo; the sample lo + u belongs to partial p = (u mod 1280) / W.  A partial starts from +0.0 and takes the terms
 *      of its samples one by one, v_p = v_p + z_t * z_(t+k), through the segments in the order of s and a segment in the order
 *      of t (terms with a +0.0 factor leave the bits of a finite sum unchanged, and the terms past hi - k are left out).  Then
 *      for off = P / 2, P / 4, .. 1 in that order v_p = v_p + v_(p+off) for every p < off, and sums = v_0.  From lambda = 640 on
 *      P = 1: one running sum.  No atomics, no scratch, asynchronous on `stream`.
 *
 *      A non-finite LIVE sample makes lag 0 of its detector non-finite and may make any other lag of that detector non-finite
 *      (Inf * +0.0 is a NaN); it touches no other detector.
 *
 *      PXL_EINVAL before any write, with a text that starts "tod_autocov" and names the argument: lambda outside 0 .. 4096; n_det,
 *      n_t or n_seg negative; n_det * n_t, n_det * (lambda + 1) or a byte count overflowing int64_t; with n_det * n_t > 0 a null
 *      x, sums or seg_start; a buffer not 8-byte aligned; sums or pairs overlapping x, wlive, seg_start or each other;
 *      n_det * ceil((lambda + 1) / W) blocks beyond 2^31 - 1.  With n_det * n_t = 0 and n_det * (lambda + 1) > 0 the outputs that
 *      are not null are still zeroed: they are overwritten outputs, not a weight.                                               */
int pxl_tod_autocov_f64(int64_t n_det, int64_t n_t, int64_t n_seg, const int64_t* seg_start, int64_t lambda, const double* x,
                        const double* wlive, double* sums, int64_t* pairs, void* stream);

/* ---- Detector pointing expansion (NOT in the reference): boresight quaternions, one per time sample, and
 *      detector offset quaternions, one per detector, to the coordinate batch sky2xN and the response batch resp2xN that
 *      every pointing entry above takes.  qbore_4xT is (w, x, y, z) of nt time samples, qdet_4xD of nd detectors, gamma_D the nd
 *      polarisation efficiencies (null: all 1); N = nd * nt and sample k = d * nt + t (detector-major).  All Float64.
 *      Quaternions are scalar first, R(q) v = q v q*, and need not be normalised: every output is invariant under q -> s q,
 *      s > 0, to rounding; the supported domain is |q_bore| |q_det| in [1e-3, 1e3].  Per sample:
 *          q = qbore[t] (x) qdet[d]  (Hamilton product),   n = R(q) z^  the line of sight,   e = R(q) x^  the sensitive direction,
 *          h = sqrt(n_x^2 + n_y^2),   ra = atan2(n_y, n_x) in (-pi, pi],   dec = atan2(n_z, h),
 *          E = (-n_y, n_x, 0) / h  (east),   N = n^ x E  (north),   c = e . N,   s = e . E,
 *          resp = gamma[d] * (c^2 - s^2, 2 c s) / (c^2 + s^2) = gamma (cos 2 psi, sin 2 psi),
 *      psi the IAU position angle of e, from north through east.  Exactly at a pole (h == 0 as computed): ra = +0.0,
 *      dec = +-pi/2, E = (0, 1, 0).  No trigonometric function is evaluated: two atan2 and one square root for the position, a
 *      reciprocal square root for the response (the closed forms in terms of q: pxl_pointing.h).  Accuracy against the same
 *      definition in long double: the great-circle separation of (ra, dec) and max(|dq|, |du|) / (gamma / h) each stay within
 *      four times what the definition evaluated in Float64 with libm reaches on the same inputs (measured: DESIGN.md 4.16); the
 *      1 / h is the conditioning of a position angle next to a pole.
 *      If any of the eight quaternion components or gamma[d] is NaN or Inf, or either quaternion is all zeros, all four
 *      outputs of that sample are NaN (the scatters add nothing for a non-finite position: a NaN boresight sample is a cut
 *      sample); no other sample is touched.  Deterministic: no atomics, every output written once, two calls on the same
 *      inputs give the same bits.
 *      PXL_EINVAL before any HIP call: nt < 0 or nd < 0, nd * nt (or its byte counts) overflowing int64_t, a null qbore_4xT,
 *      qdet_4xD, sky2xN or resp2xN with N > 0, qbore_4xT, sky2xN or resp2xN not 16-byte aligned (qdet_4xD, gamma_D: 8-byte),
 *      sky2xN or resp2xN overlapping an input or each other, more than 2^31 - 1 blocks of 256 time samples x 8 detectors.
 *      N = 0 returns 0 and launches nothing.  Asynchronous on `stream`, no synchronisation, no scratch.                    */
int pxl_pointing_expand_f64(int64_t nt, const double* qbore_4xT, int64_t nd, const double* qdet_4xD, const double* gamma_D,
                            double* sky2xN, double* resp2xN, void* stream);

/* ---- FITS image staging (the on-disk format either side of the path: read_map / write_map, enmap.jl:198-237).
 *      raw_be: device copy of the HDU's big-endian data block, n elements of BITPIX -64 (or -32 for decode);
 *      decode writes native Float64 (in place allowed for -64), encode writes big-endian Float64.          */
int pxl_fits_decode_f64(const void* raw_be, double* dst, int64_t n, int bitpix, void* stream);
int pxl_fits_encode_f64(const double* src, void* raw_be, int64_t n, void* stream);
/* BITPIX -32 <-> native Float32 (the 4-byte swap is its own inverse; in place allowed) */
int pxl_fits_swap_f32(const void* src, void* dst, int64_t n, void* stream);

/* ---- Placement probe.  The memory of a hipMalloc'ed allocation on the MI355X falls into three classes (thirds of the 288 GiB:
 *      DESIGN.md 4.7, profiles/r03_xcd_classes.txt): a kernel with several far-apart WRITE fronts -- the reprojection keeps one
 *      per XCD -- stores at 5.8-6.0 TB/s when all of them lie in one class and at 6.8-7.1 TB/s when they are split over two.
 *      This entry times the pattern that defines the classes: eight store fronts (one per XCD), four in window a and four in
 *      window b, each writing window_bytes / 4 bytes of ZEROS (both windows are overwritten).  `us` receives the median of
 *      `reps` launches in microseconds; with 1 GiB windows about 380 us = same class, 305 us = different classes.  It
 *      synchronises `stream`.  A host can map an allocation with it and put a destination across a class boundary
 *      (pixell.jl_amd/placement.py does; pxl_mem_pair_alloc below is the same rule natively).                            */
int pxl_mem_probe_pair(void* a, void* b, size_t window_bytes, int reps, float* us, void* stream);

/* A (source, destination) pair of maps placed by that rule: ONE hipMalloc of src + dst + headroom bytes (capped at the free
 * memory less 6 GiB), its classes mapped with the probe (one 1 GiB window every 2 GiB), the destination centred on the
 * boundary between two classes that has the most room on both sides, the source in a stretch of a class the destination does
 * not touch -- looked for in separate allocations (up to 96 GiB of candidates, freed again) when the allocation holds none.
 * Without a boundary inside the allocation the layout is the plain one (source first, destination at the top).  The source is
 * zero-filled; both pointers are 2 MiB aligned.  Topology discovery only: nothing about the caller's kernel is timed.  The
 * head-room stays allocated until pxl_mem_pair_free (hipMalloc cannot return part of an allocation): 144 GiB is what it takes
 * for all three classes to show up on a fresh device.  Uses the current device; synchronises `stream`.                    */
typedef struct pxl_mem_pair {
    void* src;                 /* src_bytes, zero-filled */
    void* dst;                 /* dst_bytes */
    void* arena;               /* the allocation dst (and normally src) lives in */
    void* src_alloc;           /* the separate allocation holding src, or NULL */
    uint64_t arena_bytes;
    uint64_t src_offset;       /* of src within arena (0 when src_alloc is set) */
    uint64_t dst_offset;
    int32_t classes;           /* labels given to the allocation's windows: the part has 3 classes; a window that straddles a
                                  boundary can get a label of its own */
    int32_t dst_two_classes;   /* 1: dst straddles a class boundary */
    int32_t src_own_class;     /* 1: src lies in a class dst does not touch */
    int32_t probes;            /* probe launches spent (0.3 ms each) */
    int32_t separate_tried;    /* separate source allocations tried */
    int32_t reserved_;
} pxl_mem_pair;
int pxl_mem_pair_alloc(uint64_t src_bytes, uint64_t dst_bytes, uint64_t headroom_bytes, pxl_mem_pair* out, void* stream);
int pxl_mem_pair_free(pxl_mem_pair* pair);

/* The library's DEFAULT allocation policy for a map-sized output (round 4; the reference's seam: `similar` keeps the array type,
 * src/enmap.jl:60-62, so a device host allocates its outputs through its own allocator -- this one).  ONE buffer of `bytes`
 * bytes that lies in TWO memory classes, with NO head-room kept: the buffer is allocated on its own (hipMalloc), its 1 GiB
 * windows are labelled with the probe above, and while it lies inside one class it is held as ballast and the next allocation
 * is tried (consecutive allocations walk through the device's memory; a class run is 4-32 GiB long).  A candidate with at least
 * 30 % of its windows in a second class (20 % for buffers of 16 GiB and more) is taken at once; otherwise the best one seen within `budget_bytes` of ballast (0 = 96
 * GiB; never more than the free memory less 8 GiB) and 24 tries.  All ballast is freed before the call returns.  Buffers
 * below 3 GiB are plain allocations.  The same fixed rule as pixell.jl_amd/placement.py::empty_map (what pj.reproject allocates
 * its output with); topology discovery only, nothing about the caller's kernel is timed.  Contents unspecified (probed windows
 * hold zeros).  Free with pxl_mem_free.  Uses the current device; synchronises `stream`.                                       */
typedef struct pxl_mem_placed_info {
    int32_t tries;             /* allocations made */
    int32_t probes;            /* probe launches spent */
    int32_t two_classes;       /* 1: at least 20 % of the buffer's windows lie in a second class */
    int32_t minor_share_pct;   /* share of the buffer's windows outside its majority class, in percent */
    uint64_t ballast_bytes;    /* largest amount of rejected candidates held at once (all freed on return) */
} pxl_mem_placed_info;
int pxl_mem_alloc_placed(uint64_t bytes, uint64_t budget_bytes, void** out, pxl_mem_placed_info* info, void* stream);
int pxl_mem_free(void* ptr);

/* ---- synthetic inputs (benchmark plumbing, deterministic counter-based generator):
 *      fill n doubles with N(0,1) (kind 0) or U[0,1) (kind 1) from splitmix64(seed, index+offset);
 *      uniform-on-sphere points (ra = 2pi*u1 - pi, dec = asin(2*u2 - 1)) as a 2xN batch.             */
int pxl_fill_random_f64(double* dst, int64_t n, uint64_t seed, uint64_t offset, int kind, void* stream);
int pxl_fill_sphere_points_f64(double* sky2xN, int64_t n, uint64_t seed, uint64_t offset, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PIXELL_HIP_H */
