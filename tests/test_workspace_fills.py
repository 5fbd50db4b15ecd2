"""What the byte patterns of tests/workspace_utils.py mean in every number format a workspace region is read in (fp32 residual
rows, fp16 / bf16 planes, e4m3 pieces), and that the guards' canaries can be told from both."""

import math

import pytest
import torch

import workspace_utils as wu

FORMATS = [torch.float32, torch.float16, torch.bfloat16, torch.float8_e4m3fn]


def _as(byte: int, dtype: torch.dtype) -> float:
    values = torch.full((16,), byte, dtype=torch.uint8).view(dtype).to(torch.float64)
    assert values.numel() == 16 // torch.empty((), dtype=dtype).element_size()
    assert bool((values == values[0]).all()) or bool(values.isnan().all())
    return float(values[0])


@pytest.mark.parametrize("dtype", FORMATS)
def test_the_nan_fill_is_nan_in_every_format(dtype):
    assert wu.NAN_BYTE == 0xFF
    assert math.isnan(_as(wu.NAN_BYTE, dtype))


@pytest.mark.parametrize("dtype,value,rel", [(torch.float32, 1.3058e36, 1e-4), (torch.float16, 61280.0, 0.0),
                                             (torch.bfloat16, 1.3033e36, 1e-4), (torch.float8_e4m3fn, 352.0, 0.0)])
def test_the_huge_fill_is_finite_and_large_in_every_format(dtype, value, rel):
    assert wu.HUGE_BYTE == 0x7B
    got = _as(wu.HUGE_BYTE, dtype)
    assert math.isfinite(got) and abs(got - value) <= rel * value, got
    if dtype in (torch.float16, torch.float8_e4m3fn):  # near the top of the range: squared, or summed over a row, it leaves it
        assert got > 0.75 * torch.finfo(dtype).max
    else:  # fp32's exponent range: its square is not finite in fp32
        assert got * got > torch.finfo(torch.float32).max


def test_index_and_flag_fills_are_small_integers():
    one = torch.ones(4, dtype=torch.int32)
    assert one.view(torch.uint8).tolist() == [1, 0, 0, 0] * 4
    assert torch.full((4,), wu.NAN_BYTE, dtype=torch.uint8).view(torch.int32).item() == -1  # the flag of the nan fill: raised


def test_canaries_differ_from_every_fill():
    for canary in (wu.CANARY, wu.NAN_CANARY):
        raw = torch.tensor([canary], dtype=torch.int32).view(torch.uint8).tolist()
        assert 0 <= canary < 2**31 and set(raw).isdisjoint({0x00, wu.NAN_BYTE, wu.HUGE_BYTE}), raw
    assert math.isnan(torch.tensor([wu.NAN_CANARY], dtype=torch.int32).view(torch.float32).item())


def test_fill_follows_the_layout_and_leaves_the_guards():
    layout = [{"name": "a", "offset": 0, "bytes": 300, "kind": "float"}, {"name": "m", "offset": 512, "bytes": 8, "kind": "index"},
              {"name": "f", "offset": 768, "bytes": 4, "kind": "flag"}]
    mem = wu.canaried(1024, "cpu", guard=256)
    cw = wu.ControlledWorkspace(mem, 1024, layout, 1)
    for fill, float_byte, flag in (("nan", 0xFF, -1), ("huge", 0x7B, 1)):
        wu.fill_workspace(cw, fill)
        assert bool((cw.view[:512] == float_byte).all())
        assert cw.view[512:768].view(torch.int32).tolist() == [1] * 64
        assert cw.view[768:].view(torch.int32).tolist() == [flag] * 64
        mem.assert_intact(fill)
    wu.fill_workspace(cw, "nan", only="m")
    assert bool((cw.view[:512] == 0).all()) and cw.view[512:768].view(torch.int32).tolist() == [1] * 64 and bool((cw.view[768:] == 0).all())
    wu.fill_workspace(cw, "zeros")
    assert not bool(cw.view.any())
    mem.backing[256 + 1024 + 8] = 0
    with pytest.raises(AssertionError, match="above"):
        mem.assert_intact("overrun")
