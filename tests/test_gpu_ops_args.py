"""The Python operators check a tensor's extent before anything is launched: the C ABI takes a pointer and a count, so a
malformed argument that gets past ops.py reads or writes past a buffer.  Every case here is a call that used to reach a
kernel with a count its buffers did not cover.  Each is refused with the message the same fault gets elsewhere in ops.py, leaves
the tensors the caller owns bit for bit as they were (nothing was launched), and has a well-formed neighbour that succeeds.
The kernels are not under test: 16 points, the 360 x 181 full sky and the 80 x 40 box are the smallest shapes that tell (N,)
from (N, 2) and one component from three."""
import pytest

import scatter_ref as R

torch = pytest.importorskip("torch")
from gpu_support import dev
pytestmark = pytest.mark.gpu

N = 16
SENTINEL = -7.25
BATCH = r"coordinate batches are \(N, 2\) tensors"
ONLY_CAR = "only CAR WCS"


@pytest.fixture(scope="module")
def geo(pj):
    """(full sky, box, the box's grid as a Gnomonic map)"""
    g = R.geometries(pj)
    shape, wcs = g["box_80x40"]
    return g["cc_360x181"], (shape, wcs), (shape, pj.Gnomonic(wcs.cdelt, wcs.crpix, wcs.crval))


def _full(shape, dev, value=SENTINEL):
    return torch.full(shape, value, dtype=torch.float64, device=dev)


def _points(dev, n=N):
    return torch.from_numpy(R.sphere_points(n, 0)).to(dev).contiguous()


def _untouched(t, value=SENTINEL):
    torch.cuda.synchronize()
    return bool((t.view(-1).view(torch.int64) == torch.full_like(t.view(-1), value).view(torch.int64)).all())


def test_pix2sky_rewind_takes_n_by_2_on_car(pj, dev, geo):
    full, box, tan = geo
    for g in (full, box):
        with pytest.raises(ValueError, match=BATCH):
            pj.pix2sky_rewind(g, _full((N,), dev, 3.0))                     # was passed on as 16 points: 32 doubles read and written
        with pytest.raises(ValueError, match=BATCH):
            pj.pix2sky_rewind(g, _full((N, 3), dev, 3.0))
        assert tuple(pj.pix2sky_rewind(g, _full((N, 2), dev, 3.0)).shape) == (N, 2)
    with pytest.raises(TypeError, match=ONLY_CAR):
        pj.pix2sky_rewind(tan, _full((N, 2), dev, 3.0))                     # the CAR kernel on a Gnomonic WCS


def test_vector_pairs_have_one_shape(pj, dev, geo):
    full, box, tan = geo
    a, short = _full((N,), dev, 0.1), _full((N // 2,), dev, 0.1)
    with pytest.raises(ValueError, match="ra and dec must have the same shape"):
        pj.sky2pix_broadcast(full, a, short)
    with pytest.raises(ValueError, match="ra and dec must have the same shape"):
        pj.sky2pix(tan, a, short)
    with pytest.raises(ValueError, match="ra_pixel and dec_pixel must have the same shape"):
        pj.pix2sky(tan, a, short)
    with pytest.raises(TypeError, match=ONLY_CAR):
        pj.sky2pix_broadcast(tan, a, a.clone())
    assert _untouched(a, 0.1) and _untouched(short, 0.1)
    for got in (pj.sky2pix_broadcast(full, a, a.clone()), pj.sky2pix_broadcast(box, a, a.clone()), pj.sky2pix(tan, a, a.clone()),
                pj.pix2sky(tan, a, a.clone())):
        assert len(got) == 2 and all(tuple(t.shape) == (N,) for t in got)


def test_sample_bilinear_takes_n_by_2_and_the_resident_window(pj, dev, geo):
    full, box, _tan = geo
    sky = _points(dev)
    for (shape, wcs), nc in ((full, 1), (box, 3)):
        nx, ny = shape
        m = pj.Enmap(_full((ny, nx) if nc == 1 else (nc, ny, nx), dev), wcs)
        pairs = pj.SamplePairs(m)
        with pytest.raises(ValueError, match=BATCH):
            pj.sample_bilinear(m, sky.view(-1))                             # was passed on as 32 points
        with pytest.raises(ValueError, match=BATCH):
            pj.sample_bilinear(None, sky.view(-1), pairs=pairs)
        assert tuple(pj.sample_bilinear(m, sky).shape) == (nc, N)
        assert tuple(pj.sample_bilinear(None, sky, pairs=pairs).shape) == (nc, N)
    (nx, ny), wcs = box
    half = pj.Enmap(_full((3, ny // 2, nx), dev), wcs)
    with pytest.raises(ValueError, match="is not rows"):
        pj.sample_bilinear(half, sky, src_rows=(0, ny), full_shape=(nx, ny, 3))     # 40 rows claimed, 20 resident
    assert tuple(pj.sample_bilinear(half, sky, src_rows=(0, ny // 2), full_shape=(nx, ny, 3)).shape) == (3, N)
    assert _untouched(half.data)


def test_sample_pairs_rebuild_repeats_the_window_check(pj, dev, geo):
    _full_sky, ((nx, ny), wcs), _tan = geo
    data = _full((3, ny, nx), dev, 1.5)
    pairs = pj.SamplePairs(pj.Enmap(data, wcs))
    before = pairs.data.clone()
    with pytest.raises(ValueError, match="does not match the resident window"):
        pairs.rebuild(data[:, :ny // 2].contiguous())                       # the kernel would read 40 rows of a 20-row tensor
    torch.cuda.synchronize()
    assert torch.equal(pairs.data.view(torch.int64), before.view(torch.int64))
    assert pairs.rebuild(data) is pairs


def test_generic_reproject_checks_out_without_a_plan(pj, dev, geo):
    _full_sky, ((nx, ny), wcs), (tshape, twcs) = geo
    for nc in (1, 3):
        m = pj.Enmap(_full((ny, nx) if nc == 1 else (nc, ny, nx), dev, 1.0), wcs)
        small = _full((ny // 2, nx) if nc == 1 else (nc, ny // 2, nx), dev)
        with pytest.raises(ValueError, match="out must hold %d x %d x %d elements" % (nc, ny, nx)):
            pj.reproject(m, tshape, twcs, out=pj.Enmap(small, twcs))        # was written as a whole map
        assert _untouched(small)
        out = pj.Enmap(_full(tuple(m.data.shape), dev), twcs)
        assert pj.reproject(m, tshape, twcs, out=out) is out
        assert tuple(pj.reproject(m, tshape, twcs).data.shape) == tuple(m.data.shape)


def test_fill_sphere_points_takes_n_by_2(pj, dev):
    flat = _full((N,), dev)
    with pytest.raises(ValueError, match=BATCH):
        pj.fill_sphere_points_(flat, 1)                                     # was filled as 16 points: 32 doubles
    assert _untouched(flat)
    sky = _full((N, 2), dev)
    assert pj.fill_sphere_points_(sky, 1) is sky and tuple(sky.shape) == (N, 2) and not _untouched(sky)


def test_tensors_of_one_call_live_on_one_device(pj, dev, geo):
    """The map on device 0, the points (or the second tensor) on device 1."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    other = torch.device("cuda:1")
    full, ((nx, ny), wcs), _tan = geo
    m = pj.Enmap(_full((3, ny, nx), dev, 1.0), wcs)
    sky1, a0, a1 = _points(other), _full((N,), dev, 0.1), _full((N,), other, 0.1)
    out1 = pj.Enmap(_full((3, ny, nx), other), wcs)
    plan = pj.ReprojectPlan((nx, ny, 3), wcs, (nx, ny), wcs, device=dev)
    calls = [lambda: pj.sample_bilinear(m, sky1), lambda: pj.sample_bilinear(None, sky1, pairs=pj.SamplePairs(m)),
             lambda: pj.sample(m, sky1, order=3), lambda: plan.execute(m.data, out1.data),
             lambda: plan.execute_rows(m.data, out1.data, 0, ny), lambda: pj.pix2sky(full, a0, a1), lambda: pj.sky2pix(full, a0, a1),
             lambda: pj.reproject(m, (nx, ny), wcs, out=out1, order=3)]
    for call in calls:
        with pytest.raises(ValueError, match="cuda:0"):
            call()
    torch.cuda.synchronize(other)
    assert _untouched(out1.data)
