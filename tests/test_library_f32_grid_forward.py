"""Host logic of the fp32 grid forward's dispatch (tcnn_set_fp32_grid_forward, tcnn_module_fp32_grid_forward; csrc/grid_forward_f32.hip
grid_forward_f32_is_tiled): the switch defaults to on, round-trips and leaves the other switches alone; the probe says 1 where a forward call
would run the tiled gather and 0 elsewhere; nothing a module reports about itself changes.  Both bindings.  No GPU, no compute calls."""
import pytest

from test_library_f32_fused_network import GRID, _C, _fp32, _net


@pytest.fixture(params=["compiled", "ctypes"])
def C(request, monkeypatch):
    lib = _C()
    assert lib.EXT is not None  # build() makes the compiled binding
    if request.param == "ctypes":
        monkeypatch.setattr(lib, "EXT", None)
    return lib


def test_the_switch_defaults_to_on_and_round_trips():
    C = _C()
    others = [C.get_fp32_grid_backward, C.get_fp32_fused_network, C.get_fp32_fused_backward, C.get_fp32_fused_second_order, C.get_fp32_second_order, C.get_grid_backward_mode]
    before = [get() for get in others]
    assert C.get_fp32_grid_forward() is True
    try:
        C.set_fp32_grid_forward(False)
        assert C.get_fp32_grid_forward() is False and [get() for get in others] == before
    finally:
        C.set_fp32_grid_forward(True)
    assert C.get_fp32_grid_forward() is True and [get() for get in others] == before
    for name in ("tcnn_set_fp32_grid_forward", "tcnn_get_fp32_grid_forward", "tcnn_module_fp32_grid_forward"):
        assert name in C.EXPORTED_SYMBOLS


@pytest.mark.parametrize("interpolation", ["Linear", "Smoothstep"])
@pytest.mark.parametrize("otype", ["HashGrid", "DenseGrid", "TiledGrid"])
def test_the_probe_says_1_for_fp32_grids(C, otype, interpolation):
    fp32, cfg = C.Precision.Fp32, dict(GRID, otype=otype, interpolation=interpolation)
    taken = [C.create_encoding(3, cfg, fp32),
             C.create_encoding(3, {"otype": "Composite", "nested": [dict(cfg, n_dims_to_encode=3)]}, fp32),
             C.create_network_with_input_encoding_precision(3, 4, cfg, _net(64), fp32)]
    before = [m.hyperparams() for m in taken]
    assert [(m.fp32_grid_forward(256), m.fp32_grid_forward(1 << 18), m.fp32_grid_forward(0)) for m in taken] == [(1, 1, 0)] * 3
    try:
        C.set_fp32_grid_forward(False)
        assert [m.fp32_grid_forward(256) for m in taken] == [0, 0, 0] and [m.hyperparams() for m in taken] == before
    finally:
        C.set_fp32_grid_forward(True)
    assert [m.fp32_grid_forward(256) for m in taken] == [1, 1, 1] and [m.hyperparams() for m in taken] == before


def test_the_probe_says_0_elsewhere(C):
    fp32 = C.Precision.Fp32
    assert C.create_encoding(3, dict(GRID, interpolation="Nearest"), fp32).fp32_grid_forward(256) == 0
    assert C.create_encoding(3, GRID).fp32_grid_forward(256) == 0  # 16 bits
    assert C.create_encoding(3, {"otype": "Frequency", "n_frequencies": 4}, fp32).fp32_grid_forward(256) == 0
    assert _fp32(C, 3, 4, 64).fp32_grid_forward(256) == 0  # an fp32 network without an encoding
