"""Host logic of the fused fp32 second-order pass's dispatch (csrc/mlp_kernels.h mlp_f32_backward_backward_is_fused,
tcnn_set_fp32_fused_second_order, tcnn_module_fp32_fused_second_order): the switch round-trips and defaults to on, and the query answers 0
wherever a backward_backward_input call would run the layer-by-layer launches.  No GPU, no compute calls."""
import pytest

from test_library_f32_fused_network import GRID, _C, _fp32, _net


def test_the_switch_round_trips_and_defaults_to_on():
    C = _C()
    assert C.get_fp32_fused_second_order() is True
    try:
        C.set_fp32_fused_second_order(False)
        assert C.get_fp32_fused_second_order() is False and C.get_fp32_fused_backward() is True and C.get_fp32_fused_network() is True
    finally:
        C.set_fp32_fused_second_order(True)
    assert C.get_fp32_fused_second_order() is True
    for name in ("tcnn_set_fp32_fused_second_order", "tcnn_get_fp32_fused_second_order", "tcnn_module_fp32_fused_second_order"):
        assert name in C.EXPORTED_SYMBOLS


def test_the_query_says_1_at_the_kernels_batches():
    m = _fp32(_C(), 32, 4, 64)
    assert m.fp32_fused_second_order(256) == 1 and m.fp32_fused_second_order(768) == 1 and m.fp32_fused_second_order(1 << 18) == 1


@pytest.mark.parametrize("make, n", [
    (lambda C: _fp32(C, 32, 4, 64), 128),
    (lambda C: _fp32(C, 32, 4, 48), 256),
    (lambda C: _fp32(C, 32, 4, 128), 256),
    (lambda C: C.create_network(32, 4, _net(64)), 256),
    (lambda C: C.create_encoding(3, GRID, C.Precision.Fp32), 256),
], ids=["n128", "W48", "W128", "16-bit network", "bare encoding"])
def test_the_query_says_0_where_the_layer_by_layer_launches_run(make, n):
    assert make(_C()).fp32_fused_second_order(n) == 0


@pytest.mark.parametrize("switch", ["set_fp32_fused_second_order", "set_fp32_fused_backward", "set_fp32_fused_network"])
def test_any_of_the_three_switches_turns_it_off(switch):
    C = _C()
    m = _fp32(C, 32, 4, 64)
    try:
        getattr(C, switch)(False)
        assert m.fp32_fused_second_order(256) == 0
    finally:
        getattr(C, switch)(True)
    assert m.fp32_fused_second_order(256) == 1
