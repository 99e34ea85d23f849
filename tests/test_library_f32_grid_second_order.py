"""Host logic of the fp32 grid encoding's second-order dispatch (tcnn_set_fp32_grid_second_order, tcnn_module_fp32_grid_second_order;
csrc/api_module.hip fp32_grid_second_order_route): the mask defaults to 3, round-trips, leaves the other switches alone and refuses 4; the
probe gives the bits a bwd_bwd_input call would take -- bit 0 the owner pass, bit 1 the tiled input gradient -- and 0 for everything that
is not a lone fp32 grid on the fp32 kernels.  Both bindings.  No GPU, no compute calls."""
import pytest

from test_library_f32_fused_network import GRID, _C, _net


@pytest.fixture(params=["compiled", "ctypes"])
def C(request, monkeypatch):
    lib = _C()
    assert lib.EXT is not None  # build() makes the compiled binding
    if request.param == "ctypes":
        monkeypatch.setattr(lib, "EXT", None)
    return lib


def test_the_mask_round_trips_and_refuses_4():
    C = _C()
    others = [C.get_fp32_grid_backward, C.get_fp32_grid_forward, C.get_fp32_fused_network, C.get_fp32_fused_backward, C.get_fp32_fused_second_order, C.get_fp32_second_order,
              C.get_grid_backward_mode]
    before = [get() for get in others]
    assert C.get_fp32_grid_second_order() == 1  # bit 0 on; bit 1 off (not faster at both measured grids)
    try:
        for mask in (0, 1, 2, 3):
            C.set_fp32_grid_second_order(mask)
            assert C.get_fp32_grid_second_order() == mask and [get() for get in others] == before
        for bad in (4, -1):
            with pytest.raises(RuntimeError):
                C.set_fp32_grid_second_order(bad)
            assert C.get_fp32_grid_second_order() == 3
    finally:
        C.set_fp32_grid_second_order(1)
    for name in ("tcnn_set_fp32_grid_second_order", "tcnn_get_fp32_grid_second_order", "tcnn_module_fp32_grid_second_order"):
        assert name in C.EXPORTED_SYMBOLS


def test_the_probe(C):
    fp32 = C.Precision.Fp32
    m = C.create_encoding(3, GRID, fp32)
    others = [C.create_encoding(3, GRID),  # 16 bits
              C.create_encoding(3, {"otype": "Frequency", "n_frequencies": 4}, fp32),
              C.create_encoding(3, {"otype": "Composite", "nested": [dict(GRID, n_dims_to_encode=3)]}, fp32),  # not a lone grid
              C.create_network_with_input_encoding_precision(3, 4, GRID, _net(64), fp32)]
    assert [m.fp32_grid_second_order(n) for n in (256, 768, 1 << 18, 0)] == [1, 1, 1, 0]  # the default: bit 0
    try:
        for mask in (0, 1, 2, 3):
            C.set_fp32_grid_second_order(mask)
            assert m.fp32_grid_second_order(256) == mask and m.fp32_grid_second_order(0) == 0
        assert [o.fp32_grid_second_order(256) for o in others] == [0, 0, 0, 0]
        assert C.create_encoding(3, dict(GRID, interpolation="Nearest"), fp32).fp32_grid_second_order(256) == 0
        assert C.create_encoding(3, dict(GRID, stochastic_interpolation=True), fp32).fp32_grid_second_order(256) == 2
        C.set_fp32_grid_backward(False)  # bit 0 follows the first-order switch
        assert m.fp32_grid_second_order(256) == 2
        C.set_fp32_grid_backward(True)
        C.set_fp32_second_order(1)  # the 16-bit kernels on stand-ins
        assert m.fp32_grid_second_order(256) == 0
    finally:
        C.set_fp32_second_order(0)
        C.set_fp32_grid_backward(True)
        C.set_fp32_grid_second_order(1)
    assert m.fp32_grid_second_order(256) == 1
