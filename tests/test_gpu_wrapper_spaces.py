"""The Python wrappers that take host arrays or CUDA tensors (fill_joint_track, despike_joint_track, Context.reproject,
Context.reproject_cost, PersonTracker.run_host / run_torch): the same input given once as a NumPy array and once as a CUDA tensor on a
torch stream that is not the default one gives the same bits, in the dtypes and shapes the wrappers' docstrings state.  Shapes are
the smallest that still cross the kernels' tile and staging-block edges; what the kernels compute is the business of
tests/test_gpu_fill.py, test_gpu_despike.py, test_gpu_reproject.py and test_gpu_tracking.py."""
import numpy as np
import pytest

import despike_cases as dc
import reproject_cases as rc
from test_fill_host import random_track

pytestmark = pytest.mark.gpu

LANES = (3, 5)


@pytest.fixture(scope="module")
def api():
    import snowmocap_amd as sm
    from snowmocap_amd import _lib
    assert _lib.lib().snowtri_device_count() > 0, "these tests need the HIP device"
    return sm


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.reshape(-1).view(np.uint8), b.reshape(-1).view(np.uint8))


class Side:
    """A torch stream of its own: tensors(...) uploads, `with side:` makes it torch's current stream, host(...) waits for it."""

    def __init__(self):
        import torch
        self.torch = torch
        self.stream = torch.cuda.Stream()
        assert self.stream.cuda_stream != 0
        self._cm = None

    def tensors(self, *arrays):
        out = [None if a is None else self.torch.from_numpy(np.array(a, copy=True)).cuda() for a in arrays]
        self.torch.cuda.synchronize()
        return out

    def __enter__(self):
        self._cm = self.torch.cuda.stream(self.stream)
        self._cm.__enter__()
        return self

    def __exit__(self, *exc):
        return self._cm.__exit__(*exc)

    def host(self, *tensors):
        self.stream.synchronize()
        for t in tensors:
            assert t is None or t.is_cuda
        return [None if t is None else t.cpu().numpy() for t in tensors]


# ---------------------------------------------------------------------------------------------------------------- record passes
def _record_pass_equal(run, x, codes):
    side = Side()
    h_out, h_codes = run(x, codes, None)
    assert isinstance(h_out, np.ndarray) and h_out.dtype == x.dtype and h_out.shape == x.shape
    xd, = side.tensors(x)
    with side:
        d_out, d_codes = run(xd, codes, None)                      # torch's current stream: `side`
    e_out, e_codes = run(xd, codes, side.stream.cuda_stream)       # ... and given explicitly
    d_out, d_codes, e_out, e_codes = side.host(d_out, d_codes, e_out, e_codes)
    assert _same_bits(d_out, h_out) and _same_bits(e_out, h_out)
    if codes:
        assert h_codes.dtype == np.uint8 and h_codes.shape == x.shape[:-1] and h_codes.any()
        assert _same_bits(d_codes, h_codes) and _same_bits(e_codes, h_codes)
    else:
        assert h_codes is None and d_codes is None and e_codes is None
    assert not _same_bits(h_out, x), "the pass changed nothing: the case tests nothing"


@pytest.mark.parametrize("codes", [True, False])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fill_host_array_and_tensor_agree(api, dtype, codes):
    from snowmocap_amd.fill import fill_block_frames, fill_joint_track
    T, g = fill_block_frames() + 3, 3
    x = random_track(np.random.default_rng(31), T, LANES[0] * LANES[1], g, dtype).reshape((T,) + LANES + (4,))
    _record_pass_equal(lambda a, c, s: fill_joint_track(None, a, g, codes=c, stream=s), x, codes)


@pytest.mark.parametrize("codes", [True, False])
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_despike_host_array_and_tensor_agree(api, dtype, codes):
    from snowmocap_amd.despike import DESPIKE_REPLACE, despike_joint_track
    from snowmocap_amd.fill import fill_block_frames
    T, h = fill_block_frames() + 3, 2
    e = dc.edge_track(T, LANES[0] * LANES[1], dtype, h)
    x = np.array(e["x"]).reshape((T,) + LANES + (4,))
    _record_pass_equal(lambda a, c, s: despike_joint_track(None, a, h, e["tol"], DESPIKE_REPLACE, codes=c, stream=s), x, codes)


# ---------------------------------------------------------------------------------------------------------------- reprojection
REPROJECT_SHAPE = (4, 2, 2, 5, 3)                                  # (C, P, Pmax, kn, F) of reproject_cases.cost_case


@pytest.fixture(scope="module")
def lens_context(api):
    from snowmocap_amd import _lib
    cs = rc.cost_case(REPROJECT_SHAPE)
    ctx = _lib.Context(cs["K"], cs["R"], cs["t"])
    ctx.set_distortion(cs["D"])
    yield ctx
    ctx.close()


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("pix_dtype", [None, "float32", "float64"])
@pytest.mark.parametrize("x_dtype", ["float32", "float64"])
def test_reproject_host_array_and_tensor_agree(api, lens_context, x_dtype, pix_dtype, raw):
    import torch
    C, P, _, kn, F = REPROJECT_SHAPE
    x = rc.cost_case(REPROJECT_SHAPE)["xyzs"].astype(x_dtype)
    x[1, 0, 2] = 0.0                                                                             # a missing record
    side = Side()
    host = lens_context.reproject(x, raw=raw, dtype=None if pix_dtype is None else np.dtype(pix_dtype))
    assert isinstance(host, np.ndarray) and host.dtype == np.dtype(pix_dtype or x_dtype) and host.shape == (F, C, P, kn, 3)
    assert (host[..., 2] != 0).any() and (host[..., 2] == 0).any()                               # pixels, and missing records
    xd, = side.tensors(x)
    with side:
        dev = lens_context.reproject(xd, raw=raw, dtype=None if pix_dtype is None else getattr(torch, pix_dtype))
    named = lens_context.reproject(xd, raw=raw, dtype=pix_dtype, stream=side.stream.cuda_stream)  # (a dtype by name, an explicit stream)
    dev, named = side.host(dev, named)
    assert _same_bits(dev, host) and _same_bits(named, host)


@pytest.mark.parametrize("raw", [False, True])
@pytest.mark.parametrize("with_n_persons", [True, False])
@pytest.mark.parametrize("kp_dtype", ["float32", "float64"])
def test_reproject_cost_host_arrays_and_tensors_agree(api, lens_context, kp_dtype, with_n_persons, raw):
    C, P, Pmax, kn, F = REPROJECT_SHAPE
    cs = rc.cost_case(REPROJECT_SHAPE, kp_dtype, with_n_persons)
    x, kp, npers, thr = cs["xyzs"], cs["kpts"], cs["n_persons"], cs["thr"]
    assert (npers is not None) == with_n_persons
    side = Side()
    hs, hn = lens_context.reproject_cost(x, kp, npers, thr, raw=raw)
    assert isinstance(hs, np.ndarray) and hs.dtype == np.float64 and hn.dtype == np.int32 and hs.shape == hn.shape == (F, C, P, Pmax)
    assert (hn > 0).any() and (hs > 0).any()
    xd, kd, nd = side.tensors(x, kp, npers)
    with side:
        ds, dn = lens_context.reproject_cost(xd, kd, nd, thr, raw=raw)
    es, en = lens_context.reproject_cost(xd, kd, nd, thr, raw=raw, stream=side.stream.cuda_stream)
    ds, dn, es, en = side.host(ds, dn, es, en)
    assert _same_bits(ds, hs) and _same_bits(dn, hn) and _same_bits(es, hs) and _same_bits(en, hn)


# ---------------------------------------------------------------------------------------------------------------- tracker
TRACK = dict(P=3, S=4, kn=3, cpi=1, gate=0.3, max_missed=1)


def person_lists(F, dtype, seed=5):
    """Five walkers on a 1 m lattice (jitter 0.04 m a frame), about four of them seen per frame and listed in random order: count[f]
    is often above Pout_max = 3, so the four slots fill, overflow and are re-used."""
    rng = np.random.default_rng(seed)
    P, kn, cpi = TRACK["P"], TRACK["kn"], TRACK["cpi"]
    xyzs = rng.normal(50.0, 1.0, size=(F, P, kn, 4)).astype(dtype)
    count = np.zeros(F, dtype=np.int32)
    pos = np.stack([np.arange(5.0), np.zeros(5), np.zeros(5)], axis=-1)
    for f in range(F):
        pos = pos + rng.normal(0.0, 0.04, size=pos.shape)
        seen = rng.permutation(np.nonzero(rng.random(5) < 0.75)[0])
        count[f] = len(seen)
        for p, e in enumerate(seen[:P]):
            xyzs[f, p, cpi, :3] = pos[e]
            xyzs[f, p, cpi, 3] = 0.0 if rng.random() < 0.03 else rng.uniform(0.5, 9.0)
    return xyzs, count


def _tracker():
    from snowmocap_amd.tracking import PersonTracker
    return PersonTracker(None, S=TRACK["S"], center_point_index=TRACK["cpi"], gate=TRACK["gate"], max_missed=TRACK["max_missed"])


def _track_frames():
    from snowmocap_amd.tracking import chain_block_frames
    return chain_block_frames() + 8


def _run_torch(trk, side, xyzs, count, **kw):
    xd, cd = side.tensors(xyzs, count)
    with side:
        out = trk.run_torch(xd, cd, **kw)
    keys = list(out)
    return dict(zip(keys, side.host(*[out[k] for k in keys])))


def _assert_layout(out, F, x_dtype, gather, flags_dtype):
    P, S, kn = TRACK["P"], TRACK["S"], TRACK["kn"]
    want = dict(slot_of=((F, P), np.int32), person_of=((F, S), np.int32), track_id=((F, S), np.int32), flags=((F,), flags_dtype))
    if gather:
        want["xyzs_tracked"] = ((F, S, kn, 4), x_dtype)
    assert list(out) == list(want)
    for k, (shape, dt) in want.items():
        assert out[k].shape == shape and out[k].dtype == dt, k


def _assert_same_results(a, b):
    assert list(a) == list(b)
    for k in a:                                                     # flags: uint32 from run_host, int32 from run_torch
        assert a[k].shape == b[k].shape and a[k].dtype.itemsize == b[k].dtype.itemsize and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.mark.parametrize("carry", [True, False])
@pytest.mark.parametrize("gather", [True, False])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_tracker_host_arrays_and_tensors_agree(api, dtype, gather, carry):
    F = _track_frames()
    xyzs, count = person_lists(F, dtype)
    hst, dev = _tracker(), _tracker()
    h = hst.run_host(xyzs, count, gather=gather, carry=carry)
    d = _run_torch(dev, Side(), xyzs, count, gather=gather, carry=carry)
    _assert_layout(h, F, dtype, gather, np.uint32)
    _assert_layout(d, F, dtype, gather, np.int32)
    _assert_same_results(h, d)
    assert h["track_id"].max() >= TRACK["S"] and (h["flags"] & 1).any() and (h["person_of"] < 0).any()     # births past S, overflow, empty slots
    assert np.array_equal(hst.state_blob(), dev.state_blob()) and hst.state_blob().any() == carry        # carry=False saves nothing


@pytest.mark.parametrize("first", ["host", "torch"])
def test_tracker_state_migrates_between_host_and_device(api, first):
    F = _track_frames()
    xyzs, count = person_lists(2 * F, np.float32)
    one = _tracker()
    whole = one.run_host(xyzs, count)
    mixed, side = _tracker(), Side()
    if first == "host":
        parts = [mixed.run_host(xyzs[:F], count[:F]), _run_torch(mixed, side, xyzs[F:], count[F:])]
    else:
        parts = [_run_torch(mixed, side, xyzs[:F], count[:F]), mixed.run_host(xyzs[F:], count[F:])]
    assert isinstance(mixed._state, np.ndarray) == (first == "torch")                            # the state lives where the last call's data lived
    for k in whole:                                                 # as bytes: flags are uint32 from run_host, int32 from run_torch
        assert np.array_equal(np.concatenate([p[k].reshape(-1).view(np.uint8) for p in parts]), whole[k].reshape(-1).view(np.uint8)), k
    assert np.array_equal(mixed.state_blob(), one.state_blob())
    assert len(np.unique(whole["track_id"][F:][whole["track_id"][F:] >= 0])) > 1 and whole["track_id"][F:].max() > whole["track_id"][:F].max()


def test_run_torch_names_a_malformed_tensor_in_words(api):
    """Not an AssertionError: the exceptions of the record passes and the reprojection."""
    import torch
    xyzs, count = person_lists(4, np.float32)
    xd, cd = torch.from_numpy(xyzs).cuda(), torch.from_numpy(count).cuda()
    trk = _tracker()
    with pytest.raises(ValueError, match="contiguous CUDA tensor"):
        trk.run_torch(xd[:, :, ::2], cd)                                                         # not contiguous
    with pytest.raises(ValueError, match="contiguous CUDA tensor"):
        trk.run_torch(xd.cpu(), cd)                                                              # not on the device
    with pytest.raises(ValueError):
        trk.run_torch(xd, cd.long())                                                             # count is not int32
    with pytest.raises(ValueError):
        trk.run_torch(xd, cd[:3].contiguous())                                                   # count is not [F]
    with pytest.raises(TypeError, match="float32/float64"):
        trk.run_torch(xd.half(), cd)
    with pytest.raises(ValueError, match="mixture"):
        trk.run_torch(xd, count)
    assert not trk.state_blob().any()                                                            # no refused call touched the state
