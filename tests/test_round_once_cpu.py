"""The round-once helper on constructed tensors, and the inputs of every case of tests/test_gpu_round_once.py: the reference alone
(plain torch in f32 against plain torch in f64) must stay a factor ten inside the cap the GPU pairs are held to, and must keep
every element inside its bracket -- an element that f32 evaluation noise alone moves two bf16 steps says nothing about a kernel."""
import pytest
import torch

from tests import round_once_common as RO

BF = torch.bfloat16


def _values():
    g = RO.gen(1)
    v = torch.randn(20000, generator=g) * 3
    # negative values, zeros of both signs, powers of two (the spacing halves below them) and their bf16 neighbours
    edge = torch.tensor([0.0, -0.0, 1.0, -1.0, 2.0, 0.5, -4.0, 1.0 - 2.0 ** -9, 1.0 + 2.0 ** -7, -(2.0 - 2.0 ** -8), 2.0 ** -20, -3.0e-30])
    return torch.cat([v, edge, edge * (1 + 2.0 ** -12), edge * (1 - 2.0 ** -12)])


def test_exact_roundings_pass_and_report_no_flip():
    r = _values()
    assert RO.check_round_once(r.to(BF), r, "exact") == 0.0
    assert RO.check_round_once(r.to(BF), r, "exact", cap=0.0) == 0.0
    rep = RO.r16(r)  # representable values: the bracket is a single value
    assert RO.check_round_once(rep.to(BF), rep, "representable", cap=0.0) == 0.0


def test_bracket_at_powers_of_two_zero_and_negative_values():
    r = torch.tensor([1.0 + 2.0 ** -9, 1.0 - 2.0 ** -10, -(1.0 + 2.0 ** -9), 0.0, -0.0, 3.0, 2.0 - 2.0 ** -9])
    lo, hi = RO.bracket(r)
    assert lo.tolist() == [1.0, 1.0 - 2.0 ** -8, -1.0, 0.0, -0.0, 3.0, 2.0 - 2.0 ** -7]
    assert hi.tolist() == [1.0 + 2.0 ** -7, 1.0, -(1.0 + 2.0 ** -7), 0.0, -0.0, 3.0, 2.0]
    # below 1.0 the neighbour is 2^-8 away, above it 2^-7: the far side of either is two steps and is refused
    ok = torch.tensor([1.0, 1.0]).to(BF)
    assert RO.check_round_once(ok, torch.tensor([1.0 + 2.0 ** -9, 1.0 - 2.0 ** -10]), "pow2", cap=1.0) == 0.0
    with pytest.raises(AssertionError, match="not a bf16 neighbour"):
        RO.check_round_once(torch.tensor([1.0 - 2.0 ** -8]).to(BF), torch.tensor([1.0 + 2.0 ** -9]), "pow2", cap=1.0)
    with pytest.raises(AssertionError, match="not a bf16 neighbour"):  # representable twin: only the value itself
        RO.check_round_once(torch.tensor([1.0 - 2.0 ** -8]).to(BF), torch.tensor([1.0]), "pow2", cap=1.0)
    z = torch.tensor([0.0, -0.0])
    assert RO.check_round_once(torch.tensor([-0.0, 0.0]).to(BF), z, "zero", cap=0.0) == 0.0


def test_a_second_rounding_is_reported():
    """f32 -> (value nudged across a midpoint, as an intermediate rounding does) -> bf16: the other neighbour of the bracket."""
    r = torch.tensor([1.0 + 2.0 ** -8 - 2.0 ** -20, -(2.0 + 2.0 ** -7 + 2.0 ** -19), 3.0])  # just below / above a midpoint
    twice = (r * (1 + torch.tensor([2.0 ** -16, -(2.0 ** -16), 0.0]))).to(BF)
    assert twice.float().tolist() == [1.0 + 2.0 ** -7, -2.0, 3.0] and r.to(BF).float().tolist() == [1.0, -(2.0 + 2.0 ** -6), 3.0]
    assert RO.check_round_once(twice, r, "twice", cap=1.0) == pytest.approx(2 / 3)
    with pytest.raises(AssertionError, match="differ from the rounded f32 twin"):
        RO.check_round_once(twice, r, "twice")
    # a tensor that is rounded through an intermediate format everywhere (bf16 of the f16 rounding): about 2^-4 of the roundings move
    v = _values()[:20000]
    with pytest.raises(AssertionError, match="differ from the rounded f32 twin"):
        RO.check_round_once(v.half().to(BF), v, "via f16")


@pytest.mark.parametrize("rel", [1e-3, -1e-3, 1e-4])
def test_a_systematic_relative_error_fails_the_cap(rel):
    r = _values()[:20000]
    g = (r * (1 + rel)).to(BF)
    assert RO.flip_share(g, r) > (10 if abs(rel) == 1e-3 else 1.5) * RO.CAP  # (1e-4 over a mean relative step of 2^-7.5: 1.8 %)
    with pytest.raises(AssertionError, match="differ from the rounded f32 twin"):
        RO.check_round_once(g, r, "scaled")


def test_a_two_step_element_and_a_non_finite_element_fail():
    r = _values()[:20000]
    g = r.to(BF)
    step = (RO.bracket(r)[1] - RO.bracket(r)[0])[7]
    g2 = g.clone()
    g2[7] = (g[7].float() + 2 * step.abs() * torch.sign(r[7])).to(BF)
    with pytest.raises(AssertionError, match="not a bf16 neighbour"):
        RO.check_round_once(g2, r, "two steps")
    g3 = g.clone()
    g3[9] = float("inf")
    with pytest.raises(AssertionError, match="non-finite"):
        RO.check_round_once(g3, r, "inf")
    with pytest.raises(AssertionError, match="returned"):
        RO.check_round_once(r, r, "dtype")


def test_same_f32_tolerances_and_integer_outputs():
    a = torch.randn(100, generator=RO.gen(2))
    RO.check_same_f32(a, a * (1 + 5e-5), 0, "rowln.mean")
    with pytest.raises(AssertionError):
        RO.check_same_f32(a, a * (1 + 1e-3) + 1e-4, 0, "rowln.mean")
    m = torch.randint(0, 2, (64,), dtype=torch.uint8, generator=RO.gen(3))
    RO.check_same_f32(m, m.clone(), 0, "mask")
    m2 = m.clone()
    m2[3] ^= 1
    with pytest.raises(AssertionError, match="integer elements differ"):
        RO.check_same_f32(m, m2, 0, "mask")
    with pytest.raises(AssertionError, match="storage type"):
        RO.check_same_f32(a.to(BF), a.to(BF), 0, "rowln.y")


# ---------------------------------------------------------------------------------------------------------------------------
# the inputs of the GPU cases: f32 reference against f64 reference, on every tensor the GPU test hands to check_round_once
# ---------------------------------------------------------------------------------------------------------------------------
def _inside(model, names, what):
    a, b = model(torch.float32), model(torch.float64)
    for n in names:
        far = RO.outside_bracket(a[n].to(BF), b[n].float())
        assert far == 0, f"{what} {n}: f32 evaluation noise alone moves {far} elements two bf16 steps: ill-conditioned inputs"
        share = RO.flip_share(a[n].to(BF), b[n].float())
        assert share <= RO.INPUT_CAP, f"{what} {n}: the f32 and f64 references round differently on {share:.4%} of the elements"


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("rows,cols", RO.ROWLN_SHAPES)
def test_inputs_row_layernorm(rows, cols, relu):
    inp = RO.rowln_inputs(rows, cols, RO.ROWLN_SEEDS.get((rows, cols, relu), 0))
    _inside(lambda dt: RO.rowln_model(inp, dt, relu), ("y", "dx"), f"rowln {rows}x{cols}")


def test_inputs_row_layernorm_dropout_and_grouped():
    rows, cols, p = RO.ROWLN_DROPOUT
    inp = RO.rowln_inputs(rows, cols, seed=1)
    mask = (torch.rand(rows, cols, generator=RO.gen(4)) >= p).to(torch.uint8)
    _inside(lambda dt: RO.rowln_model(inp, dt, True, mask, p), ("y", "dx"), "rowln dropout")
    ginp = RO.rowln_group_inputs()
    for k in range(len(RO.ROWLN_GROUP[1])):
        _inside(lambda dt: RO.rowln_group_model(ginp, dt)[k], ("y", "dx"), f"rowln group {k}")


@pytest.mark.parametrize("rows,cols,segs", RO.GRAPHLN_CASES)
def test_inputs_graph_layernorm(rows, cols, segs):
    inp = RO.graphln_inputs(rows, cols)
    _inside(lambda dt: RO.graphln_model(inp, dt, segs), ("y", "dx"), f"graphln {rows}x{cols}")


@pytest.mark.parametrize("cols", RO.CSR_COLS)
@pytest.mark.parametrize("kind", RO.CSR_GRAPHS)
def test_inputs_csr_gather(kind, cols):
    ei, n = RO.csr_edges(kind)
    inp = RO.csr_inputs(n, cols, RO.CSR_SEED)
    _inside(lambda dt: RO.csr_model(inp, dt, ei, n), ("fwd", "bwd"), f"csr {kind} {cols}")


@pytest.mark.parametrize("cols", RO.BANDED_COLS)
def test_inputs_banded_gather(cols):
    ei, n = RO.band_edges()
    inp = RO.csr_inputs(n, cols, RO.BAND_SEED)
    _inside(lambda dt: RO.csr_model(inp, dt, ei, n), ("fwd",), f"banded {cols}")


@pytest.mark.parametrize("cols", RO.PE_COLS)
def test_inputs_pe_add(cols):
    inp = RO.pe_inputs(cols, RO.PE_SEED)
    assert int(inp["pos"].min()) >= -64 and int(inp["pos"].max()) < 64
    _inside(lambda dt: RO.pe_model(inp, dt), ("y",), f"pe {cols}")


@pytest.mark.parametrize("n", RO.DROPOUT_N)
def test_inputs_dropout(n):
    inp = RO.dropout_inputs(n)
    mask = (torch.rand(n, generator=RO.gen(5)) >= 0.3).to(torch.uint8)
    _inside(lambda dt: RO.dropout_model(inp, dt, mask, 0.3), ("y", "dx"), f"dropout {n} p 0.3")
    exact = RO.dropout_model(inp, torch.float64, mask, 0.5)  # p = 0.5: a factor 2, no rounding at all
    assert torch.equal(RO.r16(exact["y"].float()).double(), exact["y"]) and torch.equal(RO.r16(exact["dx"].float()).double(), exact["dx"])


@pytest.mark.parametrize("M,N,K", RO.GEMM_SHAPES)
def test_inputs_contraction_epilogue(M, N, K):
    inp = RO.gemm_inputs(M, N, K, RO.GEMM_SEED)
    _inside(lambda dt: RO.gemm_model(inp, dt), ("c",), f"gemm {M}x{N}x{K}")


def test_inputs_of_the_exact_cases_are_representable():
    """Gather-max, segment-max, the casts and the gathers do no arithmetic: their activations are bf16 values, so the rounding of
    the f32 result is the value itself wherever an activation wins."""
    for k, H in RO.GATHER_MAX:
        inp = RO.gather_max_inputs(k, H)
        assert torch.equal(RO.r16(inp["f"]), inp["f"]) and torch.equal(RO.r16(inp["dm"]), inp["dm"])
    for lens, cols in RO.SEGMAX:
        inp = RO.segmax_inputs(lens, cols)
        assert all(torch.equal(RO.r16(x), x) for x in inp["xs"] + inp["douts"]) and inp["ptr"].tolist()[-1] == sum(lens)


@pytest.mark.parametrize("rows,cols", RO.HEAD_SHAPES)
@pytest.mark.parametrize("n_out", [1, 2])
def test_inputs_heads_the_designed_rounding_is_visible(rows, cols, n_out):
    """The model of the heads: the gradient rounded to bf16 before df = g W moves df by up to 2^-9 relative -- far more than the cap
    tolerates -- so a test that compares the bf16 df with the UNROUNDED model would fail: the rounding has to be modelled."""
    m = RO.head_model(RO.head_inputs(rows, cols, n_out), n_out, 0.1 if n_out == 2 else 0.0)
    assert RO.flip_share(m["df16"].float().to(BF), m["df"].float()) > 2 * RO.CAP
    rel = ((m["g16"] - m["g"]).abs() / m["g"].abs().clamp(min=1e-30)).max()
    assert float(rel) <= 2.0 ** -8
