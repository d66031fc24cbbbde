"""The buffer layer of the Python wrappers (snowmocap_amd._lib: ptr, host_floats, Space) and the argument checks the wrappers make
through it.  No GPU and no library: importing snowmocap_amd._lib loads nothing, and every check here comes before the first C call
(the contexts are dummies).  What the calls compute in the two spaces: tests/test_gpu_wrapper_spaces.py."""
import ctypes as ct

import numpy as np
import pytest
import torch

from snowmocap_amd import _lib
from snowmocap_amd._lib import Space


# ---------------------------------------------------------------------------------------------------------------- ptr
def _address(p):
    assert isinstance(p, ct.c_void_p)
    return p.value


def test_ptr_takes_what_call_sites_hold():
    class OnlyDataPtr:
        def data_ptr(self):
            return 0x1234500

    a = np.arange(6.0)
    t = torch.arange(6)
    assert _lib.ptr(None) is None
    assert _address(_lib.ptr(a)) == a.ctypes.data
    assert _address(_lib.ptr(a[2:])) == a.ctypes.data + 16
    assert _address(_lib.ptr(t)) == t.data_ptr() and t.data_ptr() != 0                           # a CPU tensor
    assert _address(_lib.ptr(OnlyDataPtr())) == 0x1234500
    assert _address(_lib.ptr(0x7f0000001000)) == 0x7f0000001000                                  # a HIP stream handle
    assert _lib.ptr(0) is None                                                                   # the null stream
    p = ct.c_void_p(4096)
    assert _lib.ptr(p) is p


# ---------------------------------------------------------------------------------------------------------------- host coercion
@pytest.mark.parametrize("via", ["host_floats", "Space.floats"])
def test_host_coercion(via):
    def coerce(a):
        if via == "host_floats":
            b = _lib.host_floats(a)
            return b, _lib.dtype_code(b.dtype)
        return Space("test").floats(a, "joints")

    for given in (np.arange(12, dtype=np.float16), np.arange(12), np.arange(12, dtype=np.float64), [[1, 2], [3, 4]], [1.5, 2.5]):
        got, code = coerce(given)
        assert got.dtype == np.float64 and code == _lib.F64 and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, np.asarray(given, dtype=np.float64))
    got, code = coerce(np.arange(12, dtype=np.float32))
    assert got.dtype == np.float32 and code == _lib.F32
    for dtype in (np.float32, np.float64):
        full = np.arange(24, dtype=dtype).reshape(4, 6)
        view = full[:, ::2]
        assert not view.flags["C_CONTIGUOUS"]
        got, _ = coerce(view)
        assert got.flags["C_CONTIGUOUS"] and got.dtype == dtype and np.array_equal(got, view) and not np.shares_memory(got, full)
        got, _ = coerce(full)
        assert got.ctypes.data == full.ctypes.data and got.dtype == dtype                        # passed through: no copy
        got, _ = coerce(full[1:3])
        assert got.ctypes.data == full[1:3].ctypes.data


def test_as_records_uses_the_same_coercion():
    from snowmocap_amd.records import as_records
    x = np.arange(2 * 3 * 5 * 4, dtype=np.float32).reshape(2, 3, 5, 4)
    full, flat, T, m = as_records(x)
    assert full is x and flat.ctypes.data == x.ctypes.data and flat.shape == (2, 15, 4) and (T, m) == (2, 15)
    full, flat, T, m = as_records(x.astype(np.int64)[:, ::2])
    assert full.dtype == np.float64 and full.shape == (2, 2, 5, 4) and flat.shape == (2, 10, 4) and flat.flags["C_CONTIGUOUS"]
    with pytest.raises(ValueError):
        as_records(np.zeros((3, 5)))


# ---------------------------------------------------------------------------------------------------------------- Space
def test_host_space_outputs_and_tail():
    sp = Space("test", np.zeros(3), None, [1, 2])
    assert sp.device is None and sp.tail() == (_lib.HOST, None)
    for kind, dtype in (("float32", np.float32), ("float64", np.float64), ("int32", np.int32), ("uint8", np.uint8), ("flags", np.uint32)):
        out = sp.empty((2, 3), kind)
        assert isinstance(out, np.ndarray) and out.dtype == dtype and out.shape == (2, 3)
    like = sp.empty_like(np.zeros((4, 2), dtype=np.float32))
    assert like.dtype == np.float32 and like.shape == (4, 2)
    assert Space("test").device is None and Space("test", None).device is None                  # no arrays: the host


def test_host_space_integer_arrays():
    sp = Space("test")
    got = sp.ints([[1, 2], [3, 4]], (2, 2), "n_persons")
    assert got.dtype == np.int32 and got.flags["C_CONTIGUOUS"] and got.tolist() == [[1, 2], [3, 4]]
    with pytest.raises(ValueError, match="n_persons"):
        sp.ints(np.zeros((2, 3), dtype=np.int32), (3, 2), "n_persons")


def test_tensor_checks_on_cpu_tensors():
    x = torch.zeros((6, 5, 4))
    sp = Space("fill_joint_track", x)
    assert sp.device == x.device
    with pytest.raises(ValueError, match="a tensor given to fill_joint_track must be a contiguous CUDA tensor"):
        sp.floats(x, "joints")
    with pytest.raises(TypeError, match="float32/float64 joints, not torch.int64"):
        sp.floats(x.long(), "joints")
    with pytest.raises(TypeError, match="float32/float64"):
        sp.floats(x.half(), "joints")
    with pytest.raises(ValueError, match="not a mixture"):
        Space("fill_joint_track", x, np.zeros(3))
    with pytest.raises(ValueError, match="not a mixture"):
        Space("Context.reproject_cost", np.zeros(3), np.zeros(3), torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="n_persons"):
        sp.ints(torch.zeros((2, 3), dtype=torch.int32), (3, 2), "n_persons")                     # wrong shape (and not CUDA)
    with pytest.raises(ValueError, match="n_persons"):
        sp.ints(torch.zeros((3, 2), dtype=torch.int64), (3, 2), "n_persons")


# ---------------------------------------------------------------------------------------------------------------- the wrappers
class DummyContext:
    """Stands where a _lib.Context would: touching the library through it is an error."""

    @property
    def L(self):
        raise AssertionError("the call reached the library")

    handle = None


def _unbound_context(C=4):
    ctx = _lib.Context.__new__(_lib.Context)                                                     # no library, no device
    ctx.C, ctx.handle = C, None
    return ctx


def _wrappers():
    """name -> call(xyzs): every wrapper that takes joint records in either space, with everything else well-formed for [3, 2, 5, 4]."""
    from snowmocap_amd.despike import despike_joint_track
    from snowmocap_amd.fill import fill_joint_track
    from snowmocap_amd.tracking import PersonTracker
    ctx = _unbound_context()
    trk = PersonTracker.__new__(PersonTracker)
    trk.ctx, trk.S, trk.cpi, trk.gate, trk.max_missed, trk.state_nbytes, trk._state = DummyContext(), 4, 1, 0.3, 0, 176, None
    like = lambda x, *shape, dtype: torch.zeros(shape, dtype=dtype) if torch.is_tensor(x) else np.zeros(shape, dtype=str(dtype).replace("torch.", ""))   # noqa: E731
    return {
        "fill_joint_track": lambda x: fill_joint_track(DummyContext(), x, 3),
        "despike_joint_track": lambda x: despike_joint_track(DummyContext(), x, 2, 0.1),
        "Context.reproject": lambda x: ctx.reproject(x),
        "Context.reproject_cost": lambda x: ctx.reproject_cost(x, like(x, 3, 4, 2, 5, 3, dtype=torch.float32), like(x, 3, 4, dtype=torch.int32)),
        "PersonTracker.run_torch": lambda x: trk.run_torch(x, like(x, 3, dtype=torch.int32)),
    }, trk


@pytest.mark.parametrize("name", ["fill_joint_track", "despike_joint_track", "Context.reproject", "Context.reproject_cost", "PersonTracker.run_torch"])
def test_every_wrapper_answers_a_mistake_with_the_same_exception(name):
    calls, trk = _wrappers()
    call = calls[name]
    x = torch.zeros((3, 2, 5, 4), dtype=torch.float64)
    with pytest.raises(ValueError, match=f"a tensor given to {name} must be a contiguous CUDA tensor"):
        call(x)                                                                                  # not on a CUDA device
    with pytest.raises(TypeError, match="float32/float64 joints, not torch.int64"):
        call(x.long())
    with pytest.raises(TypeError, match="float32/float64 joints, not torch.float16"):
        call(x.half())
    assert trk._state is None                                                                    # a refused call leaves the tracker's state alone


def test_wrappers_refuse_a_mixture_and_malformed_companions():
    ctx = _unbound_context()
    x, kp, n = np.zeros((3, 2, 5, 4)), np.zeros((3, 4, 2, 5, 3)), np.zeros((3, 4), dtype=np.int32)
    with pytest.raises(ValueError, match="not a mixture"):
        ctx.reproject_cost(x, torch.from_numpy(kp), n)
    with pytest.raises(ValueError, match="not a mixture"):
        ctx.reproject_cost(torch.from_numpy(x), torch.from_numpy(kp), n)
    with pytest.raises(ValueError, match="not a mixture"):
        ctx.reproject_cost(x, kp, torch.from_numpy(n))
    with pytest.raises(ValueError, match="n_persons"):
        ctx.reproject_cost(x, kp, np.zeros((4, 3), dtype=np.int32))                              # [C, F], not [F, C]
    with pytest.raises(ValueError, match="kpts must be"):
        ctx.reproject_cost(x, kp[:, :3], n)
    with pytest.raises(ValueError, match="xyzs must be"):
        ctx.reproject(np.zeros((3, 2, 5, 3)))
    calls, trk = _wrappers()
    with pytest.raises(ValueError, match="not a mixture"):
        trk.run_torch(torch.from_numpy(x), np.zeros(3, dtype=np.int32))
    with pytest.raises(ValueError, match="contiguous CUDA tensor"):
        trk.run_torch(x, np.zeros(3, dtype=np.int32))                                            # run_torch takes tensors
    with pytest.raises(ValueError, match="count"):
        trk.run_host(x, np.zeros(4, dtype=np.int32))                                             # count is not [F]
    with pytest.raises(ValueError, match="xyzs must be"):
        trk.run_host(np.zeros((3, 2, 5, 3)), np.zeros(3, dtype=np.int32))
    assert trk._state is None
