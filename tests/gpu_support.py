"""What the device tests (tests/test_gpu_*.py) share: the `dev` fixture, host-to-device copies, bit comparisons, the scatter
bound extended to infinite pixels, initial maps, the edge, seam and pole points, the sentinel-padded call of a raw timestream
filter entry and its sibling on device tensors, and the memory check of the tests on tens of GiB.  A test module imports what it uses; a
fixture imported into a module's namespace is found by pytest like one defined there."""
import ctypes as C
import time

import numpy as np
import pytest

import scatter_ref

torch = pytest.importorskip("torch")


def device():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import pixell_jl_amd as pj
    pj.load_library()                      # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def dev():
    return device()


def to_dev(a, dev, dtype=np.float64):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(got, want, what):
    """Same shape, NaN exactly where want is NaN (a NaN's payload is the adder's own), identical bit patterns everywhere else."""
    got = np.ascontiguousarray(got, dtype=np.float64); want = np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what + ": NaN positions differ"
    bad = (got.view(np.int64) != want.view(np.int64)) & ~nan
    assert not bad.any(), "%s: %d of %d values differ in bits (first at %d: %r against %r)" % (
        what, int(bad.sum()), bad.size, int(np.flatnonzero(bad.ravel())[0]), got.ravel()[np.flatnonzero(bad.ravel())[0]],
        want.ravel()[np.flatnonzero(bad.ravel())[0]])


def held_inf(got, ref, k, S, what):
    """scatter_ref.held, extended to infinite pixels: NaN where ref is NaN, the same infinity where ref is infinite, and the
    finite pixels within k * 2^-52 * S."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what + ": NaN pixels differ by position"
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf]), what + ": infinite pixels differ"
    fin = np.isfinite(ref)
    assert np.isfinite(S[fin]).all()
    return scatter_ref.held(np.where(fin, got, 0.0), np.where(fin, ref, 0.0), k, np.where(fin, S, 0.0), what)


def out0(nplanes, nrows, nx, seed):
    """A non-zero initial map: N(0, 1) shifted away from 0."""
    a = np.random.default_rng(seed).normal(size=(nplanes, nrows, nx))
    return a + np.copysign(0.5, a)


def out0_idle(nplanes, nrows, nx, idle, seed):
    """out0 with -0.0 and NaN alternating on up to 64 of the pixels that receive nothing (`idle`, (nrows, nx) bool)."""
    a = out0(nplanes, nrows, nx, seed)
    at = np.flatnonzero(idle.ravel())[:64]
    flat = a.reshape(nplanes, -1)
    flat[:, at[0::2]] = -0.0
    flat[:, at[1::2]] = np.nan
    return a


def edge_points(O, wcs, shape, n, seed, nonfinite_tail):
    """n points: over the map widened by 1.5 pixels (outside a box; past the seam and the pole rows of a full-sky map) and, on
    a full-sky map, half of them uniform on the sphere; then points exactly on pixel edges and centres, on the seam column, on
    the pole rows, and far outside; with nonfinite_tail the last three positions are not finite."""
    nx, ny = shape
    rng = np.random.default_rng(seed)
    if O.is_periodic(wcs, nx):
        sky = np.concatenate([scatter_ref.sphere_points(n // 2, seed), scatter_ref.box_points(O, wcs, shape, n - n // 2, seed + 1)])
    else:
        sky = scatter_ref.box_points(O, wcs, shape, n, seed + 1)
    m = min(n // 8, 400)
    if m:
        edges = np.stack([rng.integers(0, nx + 1, m) + 0.5, rng.integers(0, ny + 1, m) + 0.5], axis=1)
        edges[::2, 1] = rng.uniform(1, ny, len(edges[::2]))                       # on a column edge only
        centres = np.stack([rng.integers(1, nx + 1, m), rng.integers(1, ny + 1, m)], axis=1).astype(float)
        seam = np.stack([rng.uniform(nx, nx + 1, m), rng.uniform(1, ny, m)], axis=1)
        poles = np.stack([rng.uniform(1, nx, m), np.where(np.arange(m) % 2 == 0, 1.0, float(ny))], axis=1)
        far = np.stack([rng.uniform(-3 * nx, 4 * nx, m), rng.uniform(-2.0 * ny, -1.0, m)], axis=1)
        sky[:5 * m] = O.pix2sky(wcs, np.concatenate([edges, centres, seam, poles, far]), O.WRAP_NONE)
    if nonfinite_tail and n >= 3:
        sky[-3:] = [[np.nan, 0.1], [0.2, np.inf], [-np.inf, np.nan]]
    return sky


# ---- the raw entries of the timestream filters on buffers with sentinels on both sides of everything they write ---------------------
PAD, SENTINEL, ISENTINEL = 16, 12345.678, 0x5EA15EA1


def steps(lengths, start=0):
    """The offsets of consecutive items of these lengths, the first at `start`."""
    return [int(v) for v in np.cumsum([start] + list(lengths))]


def padded(n, dtype, dev):
    """(buf, view): n elements of dtype with PAD sentinels on both sides."""
    buf = torch.full((n + 2 * PAD,), SENTINEL if dtype == torch.float64 else ISENTINEL, dtype=dtype, device=dev)
    return buf, buf[PAD:PAD + n]


def intact(buf, n):
    b = buf.cpu().numpy()
    ref = np.full(PAD, SENTINEL if b.dtype == np.float64 else ISENTINEL, dtype=b.dtype)
    return np.array_equal(b[:PAD], ref) and np.array_equal(b[PAD + n:], ref)


def run_filter_entry(pj, dev, entry, head, d, w, n_coef, n_count, in_place=False, fit_info=True):
    """One call of the raw entry `entry`(*head, d, wfit, out, coef, count, stream) on sentinel-padded out, coef (n_coef Float64) and
    count (n_count int64).  head: the leading arguments; an array among them is uploaded as it is (int64 offsets, Float64
    couplings: no host check) and passed as its pointer.  Returns numpy (out (D, T), coef, count), the last two flat and still
    sentinels where fit_info is False."""
    d = np.ascontiguousarray(d, dtype=np.float64)
    dd = torch.from_numpy(d).to(dev)
    wd = None if w is None else to_dev(w, dev)
    held = [torch.from_numpy(a).to(dev) if isinstance(a, np.ndarray) else a for a in head]
    obuf, out = padded(d.size, torch.float64, dev)
    if in_place:
        out.copy_(dd.reshape(-1))
    cbuf, co = padded(n_coef, torch.float64, dev)
    nbuf, nu = padded(n_count, torch.int64, dev)
    p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    rc = getattr(pj.load_library(), entry)(*[p(a) if isinstance(a, torch.Tensor) else a for a in held], p(out if in_place else dd), p(wd), p(out),
                                           p(co) if fit_info else None, p(nu) if fit_info else None, None)
    assert rc == 0, pj._lib.last_error()
    torch.cuda.synchronize()
    assert intact(obuf, d.size) and intact(cbuf, n_coef) and intact(nbuf, n_count), "a sentinel was overwritten"
    if not fit_info:
        assert bool((co == SENTINEL).all()) and bool((nu == ISENTINEL).all())
    return out.cpu().numpy().reshape(d.shape), co.cpu().numpy(), nu.cpu().numpy()


def call_entry(pj, entry, *args):
    """run_filter_entry's sibling for arguments that are already on the device: one call of the raw entry `entry`(*args, stream)
    with every tensor passed as its pointer and everything else (sizes, orders, rcond_min, None for a null pointer) as it is.
    Nothing is copied, padded or downloaded."""
    rc = getattr(pj.load_library(), entry)(*[C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args], None)
    assert rc == 0, pj._lib.last_error()
    torch.cuda.synchronize()


# ---- the tests on buffers of tens of GiB (test_gpu_large_maps.py, test_gpu_large_tods.py) --------------------------------------------
GIB = 2 ** 30


def begin_large(dev, nbytes, what, cap_bytes):
    """Skip unless `nbytes` plus 8 GiB are free; start the peak-memory and wall clocks."""
    assert nbytes <= cap_bytes, "%s plans %.1f GiB: above the %d GiB every test here must fit" % (what, nbytes / GIB, cap_bytes // GIB)
    torch.cuda.empty_cache()
    free, _total = torch.cuda.mem_get_info(dev)
    if free < nbytes + 8 * GIB:
        pytest.skip("%s needs %.1f GiB of device memory plus 8 GiB; %.1f GiB are free" % (what, nbytes / GIB, free / GIB))
    torch.cuda.reset_peak_memory_stats(dev)
    return time.time()
