"""The helpers every wrapper of a library entry goes through (ishapediting_amd/_lib.py): call, scratch, tensor.

Eight-element tensors and host queries: each test is a launch or two."""
import ctypes as C

import numpy as np
import pytest
import torch

from ishapediting_amd import _lib

pytestmark = pytest.mark.gpu

A, B = 2.0, -4.0          # with the operands below every product and sum is exact in float32, fused or not


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def operands():
    x = torch.arange(8, dtype=torch.float32)
    return x, 0.5 * x + 1.0


def test_call_orders_work_on_the_callers_current_stream():
    xh, yh = operands()
    side = torch.cuda.Stream(dev())
    with torch.cuda.stream(side):
        x, y = torch.empty(8, device=dev()), torch.empty(8, device=dev())
        x.copy_(xh, non_blocking=True)                      # torch fills on the side stream ...
        y.copy_(yh, non_blocking=True)
        out = torch.empty(8, device=dev())
        _lib.call(dev(), "ishap_axpby", x.data_ptr(), y.data_ptr(), A, B, 8, out.data_ptr())      # ... the library reads there ...
        got = out.clone()                                   # ... and torch reads the result there
        assert _lib.stream_ptr(dev()) == side.cuda_stream
    side.synchronize()
    assert torch.equal(got.cpu(), A * xh + B * yh)


def test_call_with_a_fetched_stream_and_without_one():
    xh, yh = operands()
    side = torch.cuda.Stream(dev())
    first, last = C.c_int(-1), C.c_int(-1)
    with torch.cuda.stream(side):
        x, y = xh.to(dev(), non_blocking=True), yh.to(dev(), non_blocking=True)
        out = torch.empty(8, device=dev())
        _lib.call(dev(), "ishap_axpby", x.data_ptr(), y.data_ptr(), A, B, 8, out.data_ptr(), stream=side.cuda_stream)
        got = out.clone()
        # a host query that takes no stream: the bricks of a 65^3 grid that coarse cell 1 of a 5^3 volume overlaps
        _lib.call(dev(), "ishap_sparse_seed_range", 5, 65, 1, C.byref(first), C.byref(last), stream=False)
    side.synchronize()
    assert torch.equal(got.cpu(), A * xh + B * yh)
    want = C.c_int(), C.c_int()
    assert _lib.lib().ishap_sparse_seed_range(5, 65, 1, C.byref(want[0]), C.byref(want[1])) == 0
    assert (first.value, last.value) == (want[0].value, want[1].value) and 0 <= first.value <= last.value < 8


def test_a_refusal_is_a_runtime_error_with_the_librarys_words_and_the_code():
    """include/ishap.h, sparse surface: a NULL argument returns an error code and launches nothing"""
    with pytest.raises(RuntimeError) as e:
        _lib.call(dev(), "ishap_sparse_seed_volume", None, 5, 0.0, 65, None)
    words = _lib.lib().ishap_last_error().decode()
    assert "sparse seed: null argument" in words
    rc = _lib.lib().ishap_sparse_seed_volume(None, 5, 0.0, 65, None, None)
    assert rc != 0 and str(e.value) == f"libishap_hip: {words} (code {rc})"


def test_scratch_is_the_advertised_size_and_names_a_refused_entry():
    buf, nbytes = _lib.scratch(dev(), "ishap_surface_scratch_bytes", 8)
    assert nbytes == int(_lib.lib().ishap_surface_scratch_bytes(8)) > 0
    assert buf.dtype == torch.uint8 and buf.device == dev() and tuple(buf.shape) == (nbytes,)
    for sizes in ((-1, 1), (1, -1)):                        # tests/test_scratch_bytes_host.py: both answer -1
        with pytest.raises(_lib.ScratchError, match="ishap_winding_scratch_bytes") as e:
            _lib.scratch(dev(), "ishap_winding_scratch_bytes", *sizes)
        assert str(sizes) in str(e.value) and isinstance(e.value, RuntimeError)


def test_tensor_keeps_a_conforming_input_and_converts_the_rest():
    t = torch.arange(24, dtype=torch.float32, device=dev()).reshape(8, 3)
    assert _lib.tensor(t, torch.float32).data_ptr() == t.data_ptr()
    assert _lib.tensor(t, torch.float32, dev(), (-1, 3)).data_ptr() == t.data_ptr()
    a = np.arange(12, dtype=np.float64).reshape(4, 3) / 3.0
    got = _lib.tensor(a, torch.float32, dev(), (-1, 3))
    assert got.dtype == torch.float32 and got.device == dev() and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), a.astype(np.float32))
    i = torch.arange(6, dtype=torch.int64, device=dev())
    got = _lib.tensor(i, torch.int32)
    assert got.dtype == torch.int32 and got.data_ptr() != i.data_ptr() and torch.equal(got.long(), i)
    s = t[:, 1]                                             # stride 3
    got = _lib.tensor(s, torch.float32)
    assert got.is_contiguous() and got.data_ptr() != s.data_ptr() and torch.equal(got, s)
