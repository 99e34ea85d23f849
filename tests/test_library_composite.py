"""Composite and TriangleWave encodings, host side (no GPU): configuration parsing, widths and alignment (reference
encodings/composite.h:138-212, 362-400; src/encoding.cu:89-115), parameter layout, hyperparams, and the errors."""
import pytest


def _lib():
    import tinycudann
    return tinycudann._C


NET_64 = {"otype": "FullyFusedMLP", "activation": "ReLU", "output_activation": "None", "n_neurons": 64, "n_hidden_layers": 2}
NRC = {"otype": "Composite", "nested": [
    {"n_dims_to_encode": 3, "otype": "TriangleWave", "n_frequencies": 12},
    {"n_dims_to_encode": 5, "otype": "OneBlob", "n_bins": 4},
    {"otype": "Identity"},
]}
GRID = {"otype": "HashGrid", "n_levels": 2, "n_features_per_level": 4, "log2_hashmap_size": 10, "base_resolution": 4, "per_level_scale": 2.0}
MIXED = {"otype": "Composite", "nested": [
    {"n_dims_to_encode": 3, "otype": "Identity"},
    dict(GRID, n_dims_to_encode=3),
    {"n_dims_to_encode": 2, "otype": "TriangleWave", "n_frequencies": 2},
]}


@pytest.mark.parametrize("cfg", [NRC, {"otype": "NRC"}, {"otype": "OneBlobFrequency"}, {"otype": "nrc", "n_frequencies": 12, "n_bins": 4}], ids=["composite", "NRC", "OneBlobFrequency", "nrc-explicit"])
def test_nrc_encoding_on_14_inputs(cfg):
    """3 x 12 triangle waves + 5 x 4 one-blob bins + 6 identity = 62 features; 64 behind a network (the last nested encoding takes the padding)"""
    C = _lib()
    e = C.create_encoding(14, cfg)
    assert e.n_input_dims() == 14 and e.n_output_dims() == 62 and e.n_params() == 0
    assert e.name() == "CompositeEncoding"
    hp = e.hyperparams()
    assert hp == {"otype": "Composite", "nested": [{"otype": "TriangleWave", "n_frequencies": 12}, {"otype": "OneBlob", "n_bins": 4},
                                                  {"otype": "Identity", "scale": 1.0, "offset": 0.0}]}
    assert "reduction" not in hp  # composite.h:439-449
    assert [(p["dims_to_encode_begin"], p["n_dims_to_encode"], p["output_row"], p["padded_output_width"]) for p in e.nested_layout()] == [(0, 3, 0, 36), (3, 5, 36, 20), (8, 6, 56, 6)]
    m = C.create_network_with_input_encoding(14, 3, cfg, NET_64)
    assert m.n_params() == 64 * 64 + 64 * 64 + 16 * 64  # the network's only, its input 64 wide
    assert m.nested_layout()[2]["padded_output_width"] == 8
    assert m.hyperparams()["encoding"] == hp


def test_nrc_shortcut_reads_its_own_keys():
    """encoding.cu:101, 105: n_frequencies and n_bins of the shortcut's own config"""
    C = _lib()
    e = C.create_encoding(10, {"otype": "NRC", "n_frequencies": 3, "n_bins": 8})
    assert e.n_output_dims() == 3 * 3 + 5 * 8 + 2
    assert [n.get("n_frequencies", n.get("n_bins")) for n in e.hyperparams()["nested"][:2]] == [3, 8]


def test_triangle_wave_alone():
    C = _lib()
    e = C.create_encoding(3, {"otype": "TriangleWave"})
    assert e.n_output_dims() == 36 and e.n_params() == 0 and e.name() == "TriangleWaveEncoding"
    assert e.hyperparams() == {"otype": "TriangleWave", "n_frequencies": 12}
    m = C.create_network_with_input_encoding(3, 3, {"otype": "TriangleWave", "n_frequencies": 12}, NET_64)
    assert m.n_params() == 64 * 48 + 64 * 64 + 16 * 64  # 36 -> 48


def test_identity_grid_triangle_wave_alignment():
    """composite.h:188-198: nested i is padded so that nested i + 1 starts at a multiple of ITS required alignment (the grid's F = 4): the Identity
    3 -> 4; widths 4 + 8 + 4; behind a network the last nested encoding absorbs the padding to 16 (here: none needed beyond 16)"""
    C = _lib()
    e = C.create_encoding(8, MIXED)
    grid = C.create_encoding(3, GRID)
    assert e.n_output_dims() == 16 and e.n_params() == grid.n_params() > 0
    lay = e.nested_layout()
    assert [(p["output_row"], p["padded_output_width"]) for p in lay] == [(0, 4), (4, 8), (12, 4)]
    assert [(p["params_offset"], p["n_params"]) for p in lay] == [(0, 0), (0, grid.n_params()), (grid.n_params(), 0)]
    assert e.hyperparams()["nested"][1] == grid.hyperparams()
    # three frequencies: 4 + 8 + 6 = 18 bare, and the last part takes the padding to 32 behind a network
    wider = dict(MIXED, nested=MIXED["nested"][:2] + [dict(MIXED["nested"][2], n_frequencies=3)])
    assert C.create_encoding(8, wider).n_output_dims() == 18
    m = C.create_network_with_input_encoding(8, 3, wider, NET_64)
    assert [(p["output_row"], p["padded_output_width"]) for p in m.nested_layout()] == [(0, 4), (4, 8), (12, 20)]
    n_net = 64 * 32 + 64 * 64 + 16 * 64
    assert m.n_params() == n_net + grid.n_params() and m.nested_layout()[1]["params_offset"] == n_net


def test_two_grids_concatenate_their_parameters():
    C = _lib()
    g1 = dict(GRID, n_dims_to_encode=3)
    g2 = dict(GRID, n_dims_to_encode=2, n_levels=3, n_features_per_level=2)
    e = C.create_encoding(5, {"otype": "Composite", "nested": [g1, g2]})
    n1, n2 = C.create_encoding(3, GRID).n_params(), C.create_encoding(2, dict(GRID, n_levels=3, n_features_per_level=2)).n_params()
    assert e.n_params() == n1 + n2
    lay = e.nested_layout()
    assert (lay[0]["params_offset"], lay[1]["params_offset"]) == (0, n1) and lay[1]["n_params"] == n2
    assert (lay[1]["dims_to_encode_begin"], lay[1]["output_row"], e.n_output_dims()) == (3, 8, 14)
    # grid-only extras belong to a lone top-level grid
    with pytest.raises(RuntimeError):
        e.grid_level_n_params(0)


def test_sum_and_product_take_the_common_width():
    C = _lib()
    nested = [{"n_dims_to_encode": 4, "otype": "OneBlob", "n_bins": 4}, {"n_dims_to_encode": 4, "otype": "TriangleWave", "n_frequencies": 4}]
    for reduction in ("Sum", "product"):
        e = C.create_encoding(8, {"otype": "Composite", "reduction": reduction, "nested": nested})
        assert e.n_output_dims() == 16
        assert [(p["output_row"], p["padded_output_width"]) for p in e.nested_layout()] == [(0, 16), (16, 16)]
    m = C.create_network_with_input_encoding(8, 3, {"otype": "Composite", "reduction": "Sum", "nested": [dict(nested[0], n_bins=2), dict(nested[1], n_frequencies=2)]}, NET_64)
    assert [(p["output_row"], p["padded_output_width"]) for p in m.nested_layout()] == [(0, 16), (16, 16)]  # 8 -> 16 each


@pytest.mark.parametrize("cfg,n_dims,msg", [
    ({"otype": "Composite", "reduction": "Sum", "nested": [{"n_dims_to_encode": 4, "otype": "OneBlob", "n_bins": 4}, {"n_dims_to_encode": 4, "otype": "TriangleWave", "n_frequencies": 3}]}, 8,
     "equal output width"),
    ({"otype": "Composite", "reduction": "Mean", "nested": [{"otype": "Identity"}]}, 8, "Invalid reduction type"),
    ({"otype": "Composite", "nested": [{"otype": "Identity"}, {"otype": "OneBlob"}]}, 8, "may only leave 'n_dims_to_encode' unspecified for a single nested encoding"),
    ({"otype": "Composite", "nested": [{"n_dims_to_encode": 5, "otype": "Identity"}, {"n_dims_to_encode": 4, "otype": "OneBlob"}]}, 8, "must not encode more dims 9 than composite 8"),
    ({"otype": "Composite", "nested": [{"n_dims_to_encode": 4, "otype": "Composite", "nested": [{"otype": "Identity"}]}, {"otype": "Identity"}]}, 8, "nested Composite"),
    ({"otype": "Composite", "nested": [{"n_dims_to_encode": 4, "otype": "NRC"}]}, 8, "nested Composite"),
    ({"otype": "Composite", "nested": [{"n_dims_to_encode": 4, "otype": "Identity"}, {"n_dims_to_encode": 3, "dims_to_encode_begin": 2, "otype": "OneBlob"}]}, 8, "overlapping"),
    ({"otype": "Composite", "nested": [{"n_dims_to_encode": 4, "dims_to_encode_begin": 6, "otype": "Identity"}]}, 8, "reads dims"),
    ({"otype": "Composite"}, 8, "Must provide an array of nested encodings to CompositeEncoding"),
    ({"otype": "Composite", "nested": {"otype": "Identity"}}, 8, "Must provide an array of nested encodings to CompositeEncoding"),
    ({"otype": "Composite", "nested": [{"n_dims_to_encode": 3, "otype": "SphericalHarmonics"}, {"otype": "Identity"}]}, 8, "Encoding 'SphericalHarmonics' not found"),
    ({"otype": "SphericalHarmonics"}, 3, "Encoding 'SphericalHarmonics' not found"),
    ({"otype": "Composite", "nested": [{"n_dims_to_encode": 5, "otype": "HashGrid"}, {"otype": "Identity"}]}, 8, "number of input dims must be 2, 3 or 4"),
], ids=["sum-unequal", "bad-reduction", "two-unspecified", "too-many-dims", "nested-composite", "nested-nrc", "overlap", "out-of-range", "no-nested", "nested-no-array",
        "nested-sh", "sh", "nested-grid-5d"])
def test_composite_config_errors(cfg, n_dims, msg):
    import re
    C = _lib()
    C.set_log_callback(lambda sev, m: None)
    try:
        with pytest.raises(RuntimeError, match=re.escape(msg)):
            C.create_encoding(n_dims, cfg)
        with pytest.raises(RuntimeError, match=re.escape(msg)):
            C.create_network_with_input_encoding(n_dims, 3, cfg, NET_64)
    finally:
        C.set_log_callback(None)


def test_remainder_and_dropped_entries():
    """the one entry without n_dims_to_encode takes the remaining dims (also in the middle); entries left with 0 dims are dropped (composite.h:180-183)"""
    C = _lib()
    e = C.create_encoding(8, {"otype": "Composite", "nested": [{"n_dims_to_encode": 2, "otype": "Identity"}, {"otype": "OneBlob", "n_bins": 2}, {"n_dims_to_encode": 3, "otype": "Identity"}]})
    assert [(p["dims_to_encode_begin"], p["n_dims_to_encode"]) for p in e.nested_layout()] == [(0, 2), (2, 3), (5, 3)]
    e = C.create_encoding(5, {"otype": "Composite", "nested": [{"n_dims_to_encode": 5, "otype": "Identity"}, {"otype": "OneBlob"}]})
    assert len(e.nested_layout()) == 1 and e.n_output_dims() == 5
    # dims_to_encode_begin places an entry; dims nobody reads are allowed
    e = C.create_encoding(8, {"otype": "Composite", "nested": [{"n_dims_to_encode": 2, "dims_to_encode_begin": 5, "otype": "Identity"}, {"n_dims_to_encode": 1, "dims_to_encode_begin": 0, "otype": "Identity"}]})
    assert [(p["dims_to_encode_begin"], p["output_row"]) for p in e.nested_layout()] == [(5, 0), (0, 2)]


def test_more_parameter_free_parts_than_the_table_holds_are_refused():
    """the by-value part table of the fused kernels holds 16 entries (composite_kernels.h)"""
    C = _lib()
    assert C.create_encoding(16, {"otype": "Composite", "nested": [{"n_dims_to_encode": 1, "otype": "Identity"}] * 16}).n_output_dims() == 16
    with pytest.raises(RuntimeError, match="more than 16 nested encodings without parameters"):
        C.create_encoding(17, {"otype": "Composite", "nested": [{"n_dims_to_encode": 1, "otype": "Identity"}] * 17})


def test_second_order_through_a_composite_is_not_implemented():
    C = _lib()
    lib = C._lib
    e = C.create_encoding(8, MIXED)
    rc = lib.tcnn_module_backward_backward_input(e._h, None, None, 256, None, None, None, None, None, None, None)
    assert rc == 2 and b"not implemented" in lib.tcnn_last_error()  # TCNN_ERROR_UNSUPPORTED
