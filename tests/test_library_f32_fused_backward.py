"""Host logic of the fused fp32 backward pass's dispatch (csrc/mlp_kernels.h mlp_f32_backward_is_fused, tcnn_set_fp32_fused_backward,
tcnn_module_fp32_fused_backward): the switch round-trips and defaults to on, and the query answers 0 wherever a backward call would run the
layer-by-layer kernels.  No GPU, no compute calls."""
from test_library_f32_fused_network import GRID, _C, _fp32, _net


def test_the_switch_round_trips_and_defaults_to_on():
    C = _C()
    assert C.get_fp32_fused_backward() is True
    try:
        C.set_fp32_fused_backward(False)
        assert C.get_fp32_fused_backward() is False and C.get_fp32_fused_network() is True
    finally:
        C.set_fp32_fused_backward(True)
    assert C.get_fp32_fused_backward() is True
    for name in ("tcnn_set_fp32_fused_backward", "tcnn_get_fp32_fused_backward", "tcnn_module_fp32_fused_backward"):
        assert name in C.EXPORTED_SYMBOLS


def test_the_query_says_0_where_the_layer_by_layer_kernels_run():
    C = _C()
    m = _fp32(C, 32, 4, 64)
    assert m.fp32_fused_backward(256) == 1 and m.fp32_fused_backward(768) == 1 and m.fp32_fused_backward(1 << 18) == 1
    assert m.fp32_fused_backward(128) == 0
    assert C.create_network(32, 4, _net(64)).fp32_fused_backward(256) == 0
    assert C.create_encoding(3, GRID, C.Precision.Fp32).fp32_fused_backward(256) == 0
    assert _fp32(C, 32, 4, 48).fp32_fused_backward(256) == 0
    for setter in (C.set_fp32_fused_backward, C.set_fp32_fused_network):  # either switch off
        try:
            setter(False)
            assert m.fp32_fused_backward(256) == 0
        finally:
            setter(True)
        assert m.fp32_fused_backward(256) == 1
