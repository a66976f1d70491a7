"""What the five polarised map-makers ask of the operators, call by call, and what they refuse, pinned against a record (no GPU).

pj.binned_map_pol, pj.cg_map_pol, pj.binned_map_pol_nearest and the two _tod forms are host Python over ten names they look up in
ops at call time: bin_pol_nearest, scatter_pol_nearest, scatter_pol_weights_nearest, scatter_pol, scatter_pol_weights, sample_pol,
normal_pol, pol_block_solve, expand_pointing and the device gate _dev_f64.  This module replaces the ten with stand-ins on CPU
tensors (monkeypatch) and runs the map-makers end to end.  The stand-ins do cheap arithmetic of the same shape as their
counterparts -- a pixel per point from the integer coordinates (two pixels, weights 3/4 and 1/4, at order 1), accumulation into
out=, NaN and Inf passed on, A = P^T W P and a diagonal M^-1 that are positive and not proportional, so pcg takes several
iterations -- and record every call: the operator, of every tensor argument its shape, strides, dtype, a digest of its values and
which input of the case it shares storage with, every scalar and keyword, whether out=, rhs= and weights= were None or the very
object an earlier call returned, and for expand_pointing whether the two buffers are those of the previous chunk.  _dev_f64's
stand-in keeps the gate's type, dtype and contiguity checks and drops only is_cuda.

The inputs of the accumulation are small integers (responses and the order-1 weights are dyadic), so every accumulated sum is exact
and its digest is that of its bytes.  pcg's iterates are not exact, and the last bit of a dot product depends on the BLAS, so a
digest is taken of the values rounded to 2^-16 of the tensor's largest (exact for the integer sums), and info["history"] is
compared to 4 digits: the record pins which calls are made on what, not the last bits of an iteration.

Compared with tests/golden/mapmaker_call_traces.json, per case: the sequence "operator:digest of the call's record", and the record
of what the map-maker returned.  Then the refusals: one call per single fault of every map-maker, and every pair of faults on
different arguments, compared by (exception type, message): Python's check order is deterministic, so a pair has one right
answer.  A fault that only a stand-in's real counterpart refuses (a Gnomonic WCS in cg_map_pol, which scatter_pol refuses) runs
through or fails inside a stand-in; it is recorded as such and left out of the pairs.

`python tests/test_mapmaker_calls.py` records the golden file from the package in use."""
import hashlib
import itertools
import json
import math
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "mapmaker_call_traces.json")
if ROOT not in sys.path:                                  # run as a script, to record
    sys.path.insert(0, ROOT)
NX, NY = 12, 7
D, T = 3, 10
TAPS = {0: ((0, 1.0),), 1: ((0, 0.75), (1, 0.25))}
F64 = torch.float64


def _geometry(pj):
    shape, wcs = pj.fullsky_geometry((2 * math.pi / NX, math.pi / (NY - 1)))
    assert shape == (NX, NY)
    return shape, wcs


# ---- the record -------------------------------------------------------------------------------------------------------------
def _digest(t):
    """Of the values in units of 2^-16 of the largest finite one's power of two, rounded; NaN, +Inf and -Inf as marks."""
    x = t.detach().to(F64).reshape(-1)
    finite = x[torch.isfinite(x)]
    e = math.frexp(float(finite.abs().max()))[1] if finite.numel() else 0
    q = torch.nan_to_num(torch.round(x * 2.0 ** (16 - e)), nan=2.0 ** 40, posinf=2.0 ** 41, neginf=-2.0 ** 41).long()
    return hashlib.sha1(q.numpy().tobytes() + b"%d" % e).hexdigest()[:12]


class Recorder:
    def __init__(self, wcs, named):
        self.wcs, self.named = wcs, named             # named: the case's input tensors by name
        self.calls, self.returned = [], []            # returned: what every call gave back, kept alive so that `is` means it
        self.last_buffers = None

    def origin(self, v):
        """None, or 'call k' for the first call that returned this very object (alone, in a tuple, or as an Enmap's data)."""
        for k, r in enumerate(self.returned):
            for e in (r if isinstance(r, tuple) else (r,)):
                if e is v or (isinstance(v, torch.Tensor) and getattr(e, "data", None) is v):
                    return "call %d" % k
        return None

    def shares(self, t):
        p = t.untyped_storage().data_ptr()
        return sorted(k for k, n in self.named.items() if isinstance(n, torch.Tensor) and n.untyped_storage().data_ptr() == p)

    def describe(self, v, digest=True):
        if isinstance(v, torch.Tensor):
            return {"shape": list(v.shape), "strides": list(v.stride()), "dtype": str(v.dtype), "digest": digest and _digest(v),
                    "shares": self.shares(v), "is": self.origin(v)}
        if hasattr(v, "data") and hasattr(v, "wcs"):
            return {"enmap": self.describe(v.data), "wcs": self.describe(v.wcs), "is": self.origin(v)}
        if isinstance(v, (tuple, list)):
            return [self.describe(e) for e in v]
        if isinstance(v, dict):
            return {k: ["%.3e" % h for h in e] if k == "history" else self.describe(e) for k, e in v.items()}
        if v is None or isinstance(v, (bool, int, str)):
            return v
        if isinstance(v, float):
            return repr(v)
        return "the wcs" if v is self.wcs else type(v).__name__

    def wrap(self, name, fn):
        def stand_in(*args, **kw):
            call = {"op": name, "args": [self.describe(a) for a in args], "kw": {k: self.describe(v, k not in ("out_sky", "out_resp")) for k, v in sorted(kw.items()) if v is not None}}
            # (out_sky, out_resp: not yet written.  A keyword given as None is one left out: None is the default of them all.)
            if name == "expand_pointing":
                bufs = [kw[k].untyped_storage().data_ptr() for k in ("out_sky", "out_resp")]
                call["buffers of the previous chunk"] = None if args[0].storage_offset() == 0 else bufs == self.last_buffers
                self.last_buffers = bufs
            ret = fn(*args, **kw)
            call["ret"] = self.describe(ret)
            self.calls.append(call)
            self.returned.append(ret)
            return ret
        return stand_in

    def summary(self, result):
        return {"calls": ["%s:%s" % (c["op"], hashlib.sha1(json.dumps(c, sort_keys=True).encode()).hexdigest()[:10]) for c in self.calls],
                "result": self.describe(result)}


# ---- the stand-ins ----------------------------------------------------------------------------------------------------------
def _stand_ins(pj):
    Enmap = pj.Enmap

    def dev_f64(t, what):
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch tensor" % what)
        if t.dtype != F64:
            raise TypeError("%s must be float64" % what)
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % what)
        return t

    def pixels(sky, npix, order):
        base = torch.nan_to_num(sky[:, 0] + NX * sky[:, 1]).long()
        return [((base + s) % npix, a) for s, a in TAPS[order]]

    def terms(v, resp, mode):
        q, u = resp[:, 0], resp[:, 1]
        return [v, q * v, u * v] if mode == 0 else [v, q * v, u * v, q * (q * v), q * (u * v), u * (u * v)]

    def scatter(order, mode, vals, sky, resp, shape, wcs, out):
        planes = 6 if mode else 3
        if out is None:
            out = Enmap(torch.zeros((planes, shape[1], shape[0]), dtype=F64), wcs)
        dst = out.data if isinstance(out, Enmap) else out
        flat = dst.view(planes, -1)
        for c, t in enumerate(terms(vals, resp, mode)):
            for idx, a in pixels(sky, flat.shape[1], order):
                flat[c].index_add_(0, idx, a * t)
        return out if isinstance(out, Enmap) else Enmap(dst, wcs)

    def scatter_pol(vals, skycoords, resp, shape, wcs, order=1, out=None):
        return scatter(order, 0, vals, skycoords, resp, shape, wcs, out)

    def scatter_pol_weights(w, skycoords, resp, shape, wcs, order=1, out=None):
        return scatter(order, 1, w, skycoords, resp, shape, wcs, out)

    def scatter_pol_nearest(vals, skycoords, resp, shape, wcs, out=None):
        return scatter(0, 0, vals, skycoords, resp, shape, wcs, out)

    def scatter_pol_weights_nearest(w, skycoords, resp, shape, wcs, out=None):
        return scatter(0, 1, w, skycoords, resp, shape, wcs, out)

    def bin_pol_nearest(d, w, skycoords, resp, shape, wcs, rhs=None, weights=None):
        return scatter(0, 0, w * d, skycoords, resp, shape, wcs, rhs), scatter(0, 1, w, skycoords, resp, shape, wcs, weights)

    def sample_pol(m, skycoords, resp):
        flat = m.data.view(3, -1)
        q, u = resp[:, 0], resp[:, 1]
        return sum(a * ((flat[0][idx] + q * flat[1][idx]) + u * flat[2][idx]) for idx, a in pixels(skycoords, flat.shape[1], 1))

    def normal_pol(x, w, skycoords, resp, out=None):
        shape = (x.data.shape[2], x.data.shape[1])
        return scatter(1, 0, w * sample_pol(x, skycoords, resp), skycoords, resp, shape, x.wcs, out)

    def pol_block_solve(rhs, weights, rcond_min=1e-3, out=None, return_rcond=False):
        w6 = weights.data
        den = 1.0 + w6[0] + w6[3] + w6[5]
        x = rhs.data / den
        if out is None:
            res = Enmap(x, rhs.wcs)
        else:
            (out.data if isinstance(out, Enmap) else out).copy_(x)
            res = out if isinstance(out, Enmap) else Enmap(out, rhs.wcs)
        return (res, Enmap(w6[0] / den, rhs.wcs)) if return_rcond else res

    def expand_pointing(q_bore, q_det, gamma=None, out_sky=None, out_resp=None):
        nt, nd = q_bore.shape[0], q_det.shape[0]
        g = torch.ones(nd, dtype=F64) if gamma is None else gamma
        if out_sky is None:
            out_sky, out_resp = torch.empty((nd * nt, 2), dtype=F64), torch.empty((nd * nt, 2), dtype=F64)
        out_sky.view(nd, nt, 2).copy_(q_bore[None, :, 0:2] + q_det[:, None, 0:2])
        out_resp.view(nd, nt, 2).copy_(g[:, None, None] * (q_bore[None, :, 2:4] - q_det[:, None, 2:4]))
        return out_sky, out_resp

    return {"_dev_f64": dev_f64, "scatter_pol": scatter_pol, "scatter_pol_weights": scatter_pol_weights,
            "scatter_pol_nearest": scatter_pol_nearest, "scatter_pol_weights_nearest": scatter_pol_weights_nearest,
            "bin_pol_nearest": bin_pol_nearest, "sample_pol": sample_pol, "normal_pol": normal_pol, "pol_block_solve": pol_block_solve,
            "expand_pointing": expand_pointing}


def run(pj, fn, args, kw, named):
    """(Recorder, what the map-maker returned) with the ten names of ops replaced for the call."""
    from pixell_jl_amd import ops
    rec = Recorder(_geometry(pj)[1], named)
    with pytest.MonkeyPatch.context() as mp:
        for name, f in _stand_ins(pj).items():
            mp.setattr(ops, name, rec.wrap(name, f))
        return rec, getattr(pj, fn)(*args, **kw)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _ints(rng, lo, hi, size):
    return torch.from_numpy(rng.integers(lo, hi + 1, size).astype(np.float64))


def _batch(n, seed):
    """(d, w, skycoords, resp) of n points: d integers in [-8, 8], w in {1, 2, 4}, integer pixel coordinates, responses in {-1, 0, 1}."""
    rng = np.random.default_rng(seed)
    sky = torch.stack([_ints(rng, 0, NX - 1, n), _ints(rng, 0, NY - 1, n)], dim=1)
    return _ints(rng, -8, 8, n), 2.0 ** _ints(rng, 0, 2, n), sky, _ints(rng, -1, 1, (n, 2))


def _batches():
    return [_batch(n, 10 + n) for n in (1, 7, 64)]


def _observation(w_per_sample=False, with_gamma=True):
    """tod, w, q_bore, q_det, gamma of D = 3 detectors and T = 10 samples, integers (gamma dyadic)."""
    rng = np.random.default_rng(7)
    tod, w_dt, w_d = _ints(rng, -8, 8, (D, T)), 2.0 ** _ints(rng, 0, 2, (D, T)), 2.0 ** _ints(rng, 0, 2, D)
    q_bore, q_det = _ints(rng, 0, 5, (T, 4)), _ints(rng, 0, 3, (D, 4))
    gamma = torch.tensor([0.5, 1.0, 1.0], dtype=F64) if with_gamma else None
    return {"tod": tod, "w": w_dt if w_per_sample else w_d, "q_bore": q_bore, "q_det": q_det, "gamma": gamma}


def _named(batches):
    return {"batch %d %s" % (b, noun): t for b, bt in enumerate(batches) for noun, t in zip(("d", "w", "skycoords", "resp"), bt)}


CG_TOL, CG_SHORT = 1e-3, 3             # CG_SHORT: a maxiter below the iterations CG_TOL needs (asserted)


def cases(pj):
    """name -> (function, args, kw, named inputs); a fresh set of tensors on every call."""
    shape, wcs = _geometry(pj)
    out = {}
    for form in ("list", "generator", "one batch"):
        def given():
            b = _batches()[2:] if form == "one batch" else _batches()
            return (b if form != "generator" else (bt for bt in b)), _named(b)
        for fused in (True, False):
            how = "fused" if fused else "composed"
            b, named = given()
            out["binned_map_pol_nearest, %s, %s" % (form, how)] = ("binned_map_pol_nearest", (b, shape, wcs), {"fused": fused}, named)
            b, named = given()
            out["cg_map_pol, %s, %s" % (form, how)] = ("cg_map_pol", (b, shape, wcs), {"tol": CG_TOL, "fused": fused}, named)
            b, named = given()
            out["cg_map_pol, %s, %s, maxiter %d" % (form, how, CG_SHORT)] = (
                "cg_map_pol", (b, shape, wcs), {"tol": CG_TOL, "maxiter": CG_SHORT, "fused": fused}, named)
    b = _batches()
    out["binned_map_pol"] = ("binned_map_pol", b[2] + (shape, wcs), {"rcond_min": 0.01}, _named(b[2:]))
    for chunk_t, per_sample, with_gamma in itertools.product((4, 1, 10, 25, None), (False, True), (True, False)):
        o = _observation(per_sample, with_gamma)
        what = "chunk_t %s, w %s, gamma %s" % (chunk_t, "(D, T)" if per_sample else "(D,)", "(D,)" if with_gamma else "None")
        args = (o["tod"], o["w"], o["q_bore"], o["q_det"], o["gamma"], shape, wcs)
        out["binned_map_pol_nearest_tod, " + what] = ("binned_map_pol_nearest_tod", args, {"chunk_t": chunk_t}, o)
        out["cg_map_pol_tod, " + what] = ("cg_map_pol_tod", args, {"chunk_t": chunk_t, "tol": CG_TOL}, o)
    return out


def trace(pj, name):
    fn, args, kw, named = cases(pj)[name]
    rec, result = run(pj, fn, args, kw, named)
    return rec.summary(result), result


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _mutated(t, how):
    if how == "float32":
        return t.float()
    if how == "two-dimensional":
        return t[:, None].contiguous()
    if how == "another length":
        return t[:-1].contiguous()
    if how == "non-contiguous":
        return torch.stack([t, t], dim=-1)[..., 0]
    if how in ("nan", "inf"):
        t = t.clone()
        t.view(-1)[t.numel() // 2] = float(how)
        return t
    raise KeyError(how)


def _gnomonic(pj):
    return pj.Gnomonic((-0.01, 0.01), (1.0, 1.0), (0.0, 0.0))


BATCH_FORMS = ("binned_map_pol", "cg_map_pol", "binned_map_pol_nearest")
TOD_FORMS = ("binned_map_pol_nearest_tod", "cg_map_pol_tod")
SCALAR_FAULTS = {"rcond_min 0": ("rcond_min", 0.0), "rcond_min 1.5": ("rcond_min", 1.5), "rcond_min nan": ("rcond_min", float("nan")),
                 "tol 0": ("tol", 0.0), "maxiter -1": ("maxiter", -1), "chunk_t 0": ("chunk_t", 0), "chunk_t -1": ("chunk_t", -1)}


def faults(fn):
    """name -> (the argument it is a fault of, what it does to the call's arguments a)"""
    def tensor(arg, how):
        return arg, lambda a: a.__setitem__(arg, _mutated(a[arg], how))

    f = {k: (arg, lambda a, arg=arg, v=v: a.__setitem__(arg, v)) for k, (arg, v) in SCALAR_FAULTS.items()
         if arg == "rcond_min" or (arg in ("tol", "maxiter") and fn.startswith("cg_")) or (arg == "chunk_t" and fn in TOD_FORMS)}
    f["gnomonic wcs"] = ("wcs", lambda a: a.__setitem__("wcs", "gnomonic"))
    if fn in BATCH_FORMS:
        for noun in ("d", "w", "skycoords", "resp"):
            f[noun + " float32"] = tensor(noun, "float32")
        f.update({"d two-dimensional": tensor("d", "two-dimensional"), "w another length": tensor("w", "another length"),
                  "w non-contiguous": tensor("w", "non-contiguous"), "d nan": tensor("d", "nan"), "d inf": tensor("d", "inf")})
        if fn != "binned_map_pol":                      # it takes one batch as four arguments: these two cannot be written
            f["no batches"] = ("batches", lambda a: a.__setitem__("batches", "none"))
            f["a batch of three items"] = ("batches", lambda a: a.__setitem__("batches", "three items"))
    else:
        f.update({"tod float32": tensor("tod", "float32"), "w float32": tensor("w", "float32"), "w non-contiguous": tensor("w", "non-contiguous"),
                  "tod nan": tensor("tod", "nan"), "tod inf": tensor("tod", "inf"),
                  "tod one-dimensional": ("tod", lambda a: a.__setitem__("tod", a["tod"][0].contiguous())),
                  "tod with T = 0": ("tod", lambda a: a.__setitem__("tod", a["tod"][:, :0].contiguous())),
                  "w of shape (D - 1,)": tensor("w", "another length"),
                  "q_bore with T - 1 rows": tensor("q_bore", "another length"),
                  "q_det with D + 1 rows": ("q_det", lambda a: a.__setitem__("q_det", torch.cat([a["q_det"], a["q_det"][:1]]))),
                  "q_det as a list": ("q_det", lambda a: a.__setitem__("q_det", a["q_det"].tolist()))})
    return f


def answer(pj, fn, *mutations):
    """[exception type, message] of the map-maker `fn` on good arguments after `mutations`; ["returns", ""] when it runs through and
    ["in a stand-in", type] when the exception is not the driver's: raised in this file, where the real operator has checks (the
    gate's stand-in apart: its refusals are the gate's own)."""
    shape, wcs = _geometry(pj)
    a = {"wcs": wcs, "batches": "all", "rcond_min": 1e-3, "tol": CG_TOL, "maxiter": 200, "chunk_t": 4}
    if fn in BATCH_FORMS:
        a.update(zip(("d", "w", "skycoords", "resp"), _batches()[1]))          # the faults go into the middle batch of three
    else:
        a.update(_observation())
    for _arg, mutate in mutations:
        mutate(a)
    if a["wcs"] == "gnomonic":
        a["wcs"] = _gnomonic(pj)
    bt = (a.get("d"), a.get("w"), a.get("skycoords"), a.get("resp"))
    b = _batches()
    batches = {"all": [b[0], bt, b[2]], "none": [], "three items": [b[0], bt[:3], b[2]]}[a["batches"]]
    kw = {"rcond_min": a["rcond_min"]}
    if fn.startswith("cg_"):
        kw.update(tol=a["tol"], maxiter=a["maxiter"])
    if fn == "binned_map_pol":
        args = bt + (shape, a["wcs"])
    elif fn in BATCH_FORMS:
        args = (batches, shape, a["wcs"])
    else:
        args, kw["chunk_t"] = (a["tod"], a["w"], a["q_bore"], a["q_det"], a["gamma"], shape, a["wcs"]), a["chunk_t"]
    try:
        run(pj, fn, args, kw, {})
    except Exception as e:
        tb = e.__traceback__
        while tb.tb_next is not None:
            tb = tb.tb_next
        if os.path.abspath(tb.tb_frame.f_code.co_filename) == os.path.abspath(__file__) and tb.tb_frame.f_code.co_name != "dev_f64":
            return ["in a stand-in", type(e).__name__]
        return [type(e).__name__, str(e)]
    return ["returns", ""]


def single_answers(pj, fn):
    return {name: answer(pj, fn, m) for name, m in faults(fn).items()}


def pair_answers(pj, fn, singles):
    """'f+g' -> answer for every two faults on different arguments that the driver itself refuses"""
    fs = faults(fn)
    live = [k for k in fs if singles[k][0] not in ("returns", "in a stand-in")]
    return {"%s+%s" % (f, g): answer(pj, fn, fs[f], fs[g]) for f, g in itertools.combinations(live, 2) if fs[f][0] != fs[g][0]}


# ---- the tests --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _case_names():
    import pixell_jl_amd as pj
    return sorted(cases(pj))


def test_the_record_covers_the_cases(pj, golden):
    assert sorted(golden["traces"]) == sorted(cases(pj)) and sorted(golden["singles"]) == sorted(BATCH_FORMS + TOD_FORMS)


@pytest.mark.parametrize("name", _case_names())
def test_the_operator_calls_are_as_recorded(pj, golden, name):
    got, result = trace(pj, name)
    want = golden["traces"][name]
    first = next((k for k, (g, w) in enumerate(zip(got["calls"], want["calls"])) if g != w), min(len(got["calls"]), len(want["calls"])))
    assert got["calls"] == want["calls"], "%d calls against %d recorded; the first that differs is call %d: %s against %s" % (
        len(got["calls"]), len(want["calls"]), first, got["calls"][first:first + 1], want["calls"][first:first + 1])
    assert got["result"] == want["result"]
    if name.startswith("cg_"):                          # what the cases are there for: several iterations, and a cap that bites
        info = result[2]
        capped = "maxiter" in name
        assert not info["breakdown"] and info["converged"] == (not capped)
        assert info["iterations"] == CG_SHORT if capped else info["iterations"] > CG_SHORT


def test_the_chunks_are_views_of_two_buffers(pj):
    """Read from the trace itself, not from the record: with chunk_t = 4 of T = 10 every expansion after a pass's first writes the
    buffers of the chunk before it, and bin_pol_nearest takes a copy of the samples (chunk_t = 10: tod itself)."""
    for chunk_t, shares in ((4, []), (10, ["tod"])):
        o = _observation()
        shape, wcs = _geometry(pj)
        rec, _res = run(pj, "binned_map_pol_nearest_tod", (o["tod"], o["w"], o["q_bore"], o["q_det"], o["gamma"], shape, wcs), {"chunk_t": chunk_t}, o)
        expands = [c for c in rec.calls if c["op"] == "expand_pointing"]
        assert [c["buffers of the previous chunk"] for c in expands] == [None, True, True][:len(expands)]
        bins = [c for c in rec.calls if c["op"] == "bin_pol_nearest"]
        assert len(bins) == len(expands) and all(c["args"][0]["shares"] == shares for c in bins)
        assert [c["kw"].get("rhs") and c["kw"]["rhs"]["is"] for c in bins] == [None] + ["call %d" % rec.calls.index(bins[0])] * (len(bins) - 1)


@pytest.mark.parametrize("fn", BATCH_FORMS + TOD_FORMS)
def test_single_faults_are_refused_as_recorded(pj, golden, fn):
    got, want = single_answers(pj, fn), golden["singles"][fn]
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


@pytest.mark.parametrize("fn", BATCH_FORMS + TOD_FORMS)
def test_two_faults_are_refused_as_recorded(pj, golden, fn):
    got = pair_answers(pj, fn, single_answers(pj, fn))
    want = {k: golden["answers"][i] for k, i in golden["pairs"][fn].items()}
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong


def _record():
    import pixell_jl_amd as pj
    traces = {name: trace(pj, name)[0] for name in sorted(cases(pj))}
    singles = {fn: single_answers(pj, fn) for fn in BATCH_FORMS + TOD_FORMS}
    answers, pairs = [], {}
    for fn in BATCH_FORMS + TOD_FORMS:
        pairs[fn] = {}
        for key, got in pair_answers(pj, fn, singles[fn]).items():
            if got not in answers:
                answers.append(got)
            pairs[fn][key] = answers.index(got)
    with open(GOLDEN, "w") as f:
        json.dump({"traces": traces, "singles": singles, "pairs": pairs, "answers": answers}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("recorded %d operator calls of %d cases, %d single faults, %d pairs of faults"
          % (sum(len(t["calls"]) for t in traces.values()), len(traces), sum(len(s) for s in singles.values()), sum(len(p) for p in pairs.values())))


if __name__ == "__main__":
    _record()
