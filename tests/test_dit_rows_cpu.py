"""The coverage contract of tests/test_gpu_dit_rows.py for layernorm_mod_kernel<MAXC>, checked without a GPU: its table of cases reaches all
five instantiations, every hidden size of the real PixArt / Flux models runs the instantiation it takes at that very width, and the ladder of
thresholds is where the table assumes.  Host arithmetic only (gdf_op_layernorm_mod_path, which the launcher itself calls)."""
from ops_binding import lib
from test_gpu_dit_rows import LN_CASES

from components import native


def test_cases_reach_every_instantiation():
    L = lib()
    assert {L.gdf_op_layernorm_mod_path(c["C"]) for c in LN_CASES} == {1, 2, 4, 6, 8}
    for c in LN_CASES:
        assert L.gdf_op_layernorm_mod_path(c["C"]) == c["maxc"], c["id"]
    assert len({c["id"] for c in LN_CASES}) == len(LN_CASES)


def test_every_model_width_has_a_case():
    L = lib()
    widths = {cfg["num_attention_heads"] * cfg["attention_head_dim"] for cfgs in (native.PIXART_CONFIGS, native.FLUX_CONFIGS) for cfg in cfgs.values()}
    assert widths
    for C in widths:
        assert L.gdf_op_layernorm_mod_path(C) in (1, 2, 4, 6, 8)
        assert any(c["C"] == C and c["maxc"] == L.gdf_op_layernorm_mod_path(C) for c in LN_CASES), C


def test_ladder_boundaries():
    L = lib()
    path = L.gdf_op_layernorm_mod_path
    assert [path(C) for C in (8, 512, 520, 1024, 1032, 2048, 2056, 3072, 3080, 4096)] == [1, 1, 2, 2, 4, 4, 6, 6, 8, 8]
    assert path(4104) == 0 and path(12) == 0 and path(0) == 0 and path(-8) == 0
