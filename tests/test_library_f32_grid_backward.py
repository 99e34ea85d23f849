"""Host logic of the fp32 grid backward's dispatch (tcnn_set_fp32_grid_backward, tcnn_module_fp32_grid_backward: host arithmetic on
csrc/grid_backward_plan.h make_f32_backward_plan): the switch defaults to on, round-trips and leaves the other switches alone; the probe says 1
where a backward call would send a grid level through the owner pass and 0 elsewhere.  Both bindings.  No GPU, no compute calls."""
import pytest

from test_library_f32_fused_network import GRID, _C, _net


@pytest.fixture(params=["compiled", "ctypes"])
def C(request, monkeypatch):
    lib = _C()
    assert lib.EXT is not None  # build() makes the compiled binding
    if request.param == "ctypes":
        monkeypatch.setattr(lib, "EXT", None)
    return lib


def test_the_switch_defaults_to_on_and_round_trips():
    C = _C()
    others = [C.get_fp32_fused_network, C.get_fp32_fused_backward, C.get_fp32_fused_second_order, C.get_fp32_second_order, C.get_grid_backward_mode]
    before = [get() for get in others]
    assert C.get_fp32_grid_backward() is True
    try:
        C.set_fp32_grid_backward(False)
        assert C.get_fp32_grid_backward() is False and [get() for get in others] == before
    finally:
        C.set_fp32_grid_backward(True)
    assert C.get_fp32_grid_backward() is True and [get() for get in others] == before
    for name in ("tcnn_set_fp32_grid_backward", "tcnn_get_fp32_grid_backward", "tcnn_module_fp32_grid_backward"):
        assert name in C.EXPORTED_SYMBOLS


def test_the_probe(C):
    fp32 = C.Precision.Fp32
    taken = [C.create_encoding(3, GRID, fp32),
             C.create_encoding(3, {"otype": "Composite", "nested": [dict(GRID, n_dims_to_encode=3)]}, fp32),
             C.create_network_with_input_encoding_precision(3, 4, GRID, _net(64), fp32)]
    for m in taken:
        assert m.fp32_grid_backward(256) == 1 and m.fp32_grid_backward(768) == 1 and m.fp32_grid_backward(1 << 18) == 1 and m.fp32_grid_backward(0) == 0
    assert C.create_encoding(3, GRID).fp32_grid_backward(256) == 0  # 16 bits
    assert C.create_encoding(3, {"otype": "Frequency", "n_frequencies": 4}, fp32).fp32_grid_backward(256) == 0
    assert C.create_encoding(3, dict(GRID, stochastic_interpolation=True), fp32).fp32_grid_backward(256) == 0
    try:
        C.set_fp32_grid_backward(False)
        assert [m.fp32_grid_backward(256) for m in taken] == [0, 0, 0]
    finally:
        C.set_fp32_grid_backward(True)
    assert [m.fp32_grid_backward(256) for m in taken] == [1, 1, 1]
