"""GemmArgs::k_period on the 256x128 split-K weight-gradient engine, and GemmArgs::colsum_row_period on
the 256x256 engines' x-aux epilogue (last_cls_bwd).

The caller promises that rows k of the M-contiguous A operand with k % k_period != 0 are exact zeros;
the engine then walks only the 32-row K-steps that hold a row i * k_period, with the dense call's split
count, slabs and reduce.  A skipped step would have added products of exact zeros to an fp32 accumulator
that starts at +0 and can never be -0, so every check here is bit for bit (no tolerance).

Shapes: one 256x128 tile and 2 x 2 tiles; K = 4096 and 6304 (= 32 x 197, the trainer's B = 32 token
count); periods 33 (the smallest the engine honours: every step but one in 33 still runs), 64 (every
other step) and 197 (the trainer's T: period rows at every offset inside a step); split-K 1 (the
accumulate-in-place epilogue into a non-zero C), 3 and 4 (slabs; 6304 / 3 gives a chunk of 2112 rows
and 4096 / 4 one of 1024, so chunk boundaries fall before, on (64 | 1024) and after a period row, and
with period 197 some steps of a chunk are the first or last of it).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PERIODS = (33, 64, 197)
SPLITS = (1, 3, 4)
SHAPES = [(256, 128, 4096), (256, 128, 6304), (512, 256, 4096), (512, 256, 6304)]


def D(vit, a, dtype):
    return vit.DeviceArray.from_numpy(np.ascontiguousarray(a, dtype=dtype))


_cache = {}


def _operands(v, M, N, K):
    """bf16 bit patterns: A [K][M] (M-contiguous), B [K][N] (N-contiguous), and a non-zero fp32 C."""
    key = (M, N, K)
    if key not in _cache:
        rng = np.random.default_rng(M + 3 * N + 7 * K)
        a = v.bf16_bits(rng.normal(size=(K, M)).astype(np.float32)).reshape(K, M)
        b = v.bf16_bits(rng.normal(size=(K, N)).astype(np.float32)).reshape(K, N)
        c = rng.normal(size=(M, N)).astype(np.float32)
        for x in (a, b, c):
            x.setflags(write=False)
        _cache[key] = (a, b, c)
    return _cache[key]


def _masked(a, period, neg_zero=False):
    """A with every row off the period rows zeroed (+0, or alternately -0: what a LayerNorm backward may
    leave, and still an exact zero)."""
    out = np.zeros_like(a)
    if neg_zero:
        out[1::2] = 0x8000
    out[::period] = a[::period]
    return out


def _run(v, a, Bd, c, M, N, K, splitk, k_period):
    out = D(v, c, np.float32)
    v.call("gemm_bf16_kperiod", out, N, D(v, a, np.uint16), M, 0, Bd, N, 0, M, N, K, 2, splitk, k_period)
    return out.numpy().reshape(M, N)


def _bits_equal(x, y):
    return np.array_equal(x.view(np.uint32), y.view(np.uint32))


def _hits_g4(v):
    return int(v.kernel_hits()[v.HIT_GEMM_256x128:v.HIT_GEMM_256x128 + 16].sum())


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_kperiod_equals_dense(gpu, M, N, K):
    """A non-zero on the period rows only: the k_period call equals the dense call bit for bit, and both
    ran on the 256x128 engine."""
    v = gpu
    a, b, c = _operands(v, M, N, K)
    Bd = D(v, b, np.uint16)
    for period in PERIODS:
        am = _masked(a, period, neg_zero=period == 197)
        for splitk in SPLITS:
            h0 = _hits_g4(v)
            dense = _run(v, am, Bd, c, M, N, K, splitk, 0)
            skip = _run(v, am, Bd, c, M, N, K, splitk, period)
            assert _hits_g4(v) == h0 + 2, "not on the 256x128 engine"
            assert np.isfinite(skip).all()
            assert not _bits_equal(skip, c), "nothing was accumulated"
            assert _bits_equal(skip, dense), (period, splitk, int(np.sum(skip != dense)))


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_kperiod_really_skips(gpu, M, N, K):
    """A random everywhere: the k_period call equals the dense call on A with the other rows zeroed, up
    to the rows that share a walked K-step with a period row.  Those the engine reads, so the reference
    keeps them: the rows of [(i * period) & ~31, + 32).  An implementation that ignores the field adds
    every row and fails."""
    v = gpu
    a, b, c = _operands(v, M, N, K)
    Bd = D(v, b, np.uint16)
    for period in PERIODS:
        keep = np.zeros(K, bool)
        for r in range(0, K, period):
            keep[(r & ~31):(r & ~31) + 32] = True
        assert not keep.all()
        aw = np.where(keep[:, None], a, np.uint16(0))
        for splitk in SPLITS:
            want = _run(v, aw, Bd, c, M, N, K, splitk, 0)
            got = _run(v, a, Bd, c, M, N, K, splitk, period)
            full = _run(v, a, Bd, c, M, N, K, splitk, 0)
            assert _bits_equal(got, want), (period, splitk, int(np.sum(got != want)))
            assert not _bits_equal(got, full), (period, splitk)


@pytest.mark.parametrize("M,N,K", SHAPES[:2])
def test_period_of_one_step_runs_dense(gpu, M, N, K):
    """k_period = 32 (not above the engine's K-step) is ignored: A random everywhere, the dense result."""
    v = gpu
    a, b, c = _operands(v, M, N, K)
    Bd = D(v, b, np.uint16)
    for splitk in SPLITS:
        assert _bits_equal(_run(v, a, Bd, c, M, N, K, splitk, 32), _run(v, a, Bd, c, M, N, K, splitk, 0))


def test_other_engines_run_dense(gpu):
    """A shape the 256x128 engine does not take (M = 128): the field is ignored, A random everywhere."""
    v = gpu
    M, N, K = 128, 128, 4096
    a, b, c = _operands(v, M, N, K)
    Bd = D(v, b, np.uint16)
    assert _bits_equal(_run(v, a, Bd, c, M, N, K, 0, 197), _run(v, a, Bd, c, M, N, K, 0, 0))


# ------------------------------------------------------------------ colsum_row_period (epi 9)
T_ROWS = 197


def _fused_rows(v, C, aux, ldx, A, lda, W, colsum, M, N, K, gathered, period):
    v.call("gemm_bf16_fused_rows", C, None, ldx, aux, ldx, A, lda, 1, W, K, 1, None, colsum, M, N, K, 9,
           gathered, period)


def _epi9_case(v, Bm, K, N=256, T=T_ROWS):
    """The dense tensor of Bm * T rows: A non-zero on rows i * T only, aux random everywhere but -0.0 in
    the even columns of row 0, so those products are zeros of the accumulator's opposite sign: -0.0
    wherever the accumulator is positive."""
    rng = np.random.default_rng(Bm * 31 + K)
    R = Bm * T
    a = np.zeros((R, K), np.uint16)
    a[::T] = v.bf16_bits(rng.normal(size=(Bm, K)).astype(np.float32)).reshape(Bm, K)
    aux = v.bf16_bits(rng.normal(size=(R, N)).astype(np.float32)).reshape(R, N).copy()
    aux[0, ::2] = 0x8000
    w = v.bf16_bits((rng.normal(size=(N, K)) * 0.1).astype(np.float32)).reshape(N, K)
    cs0 = rng.normal(size=N).astype(np.float32)
    return a, aux, w, cs0


@pytest.mark.parametrize("K", [64, 256])
@pytest.mark.parametrize("Bm", [1, 3, 4, 260])
def test_colsum_row_period_equals_full_size(gpu, Bm, K):
    """The gathered call (M = Bm, strides x T, colsum_row_period = T) against the full-size call on the
    256x256 engine: output rows i * T and colsum_out bit for bit; the rows in between are not written.
    Bm = 1, 3, 4: one ragged row panel; 260: two row tiles, the second ragged."""
    v = gpu
    N, T = 256, T_ROWS
    R = Bm * T
    a, aux, w, cs0 = _epi9_case(v, Bm, K)
    A, X, W = D(v, a, np.uint16), D(v, aux, np.uint16), D(v, w, np.uint16)
    h0 = int(v.kernel_hits()[v.HIT_GEMM_256x256 + 9])
    c_full, cs_full = D(v, np.full((R, N), 0x7FC0), np.uint16), D(v, cs0, np.float32)
    _fused_rows(v, c_full, X, N, A, K, W, cs_full, R, N, K, 1, 0)
    fill = 0x3F80  # 1.0: what the gathered call must leave in the rows it skips
    c_g, cs_g = D(v, np.full((R, N), fill), np.uint16), D(v, cs0, np.float32)
    _fused_rows(v, c_g, X, T * N, A, T * K, W, cs_g, Bm, N, K, 1, T)
    assert int(v.kernel_hits()[v.HIT_GEMM_256x256 + 9]) == h0 + 2, "not on the 256x256 engine"
    full = c_full.numpy().reshape(R, N)
    got = c_g.numpy().reshape(R, N)
    assert np.array_equal(got[::T], full[::T])
    assert (full[0, ::2] & 0x7FFF == 0).all() and (full[0, ::2] == 0x8000).sum() >= 16, "the -0.0 products"
    mask = np.ones(R, bool)
    mask[::T] = False
    assert (got[mask] == fill).all() and (full[mask] & 0x7FFF == 0).all()
    s_full, s_g = cs_full.numpy(), cs_g.numpy()
    assert np.isfinite(s_g).all() and not np.array_equal(s_g, cs0)
    assert np.array_equal(s_g.view(np.uint32), s_full.view(np.uint32)), int(np.sum(s_g != s_full))


def test_colsum_row_period_below_block_height_rejected(gpu):
    """period = 100 < 128: two gathered rows could share a partial row, so the call is an error."""
    v = gpu
    Bm, K, N = 4, 64, 256
    a, aux, w, cs0 = _epi9_case(v, Bm, K, T=100)
    A, X, W = D(v, a, np.uint16), D(v, aux, np.uint16), D(v, w, np.uint16)
    c, cs = D(v, np.zeros((Bm * 100, N)), np.uint16), D(v, cs0, np.float32)
    with pytest.raises(v.VitError):
        _fused_rows(v, c, X, 100 * N, A, 100 * K, W, cs, Bm, N, K, 1, 100)
    assert np.array_equal(cs.numpy(), cs0)
