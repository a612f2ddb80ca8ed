"""The field MLP (csrc/field.hip) and its training kernels (csrc/
field_train.hip) against an independent numpy restatement on a network whose
arithmetic is exact (tests/field_exact.py): inference bit for bit, gradients
element by element within a derived fp32 summation bound."""
import numpy as np
import pytest

import field_exact as fx

EPS32 = 2.0 ** -24


# ------------------------------------------------------------------ CPU ----
@pytest.mark.parametrize("n_hidden", [0, 1, 4, 16])
@pytest.mark.parametrize("n_in", [23, 38, 54, 64])
def test_recipe_is_order_independent(n_in, n_hidden):
    """The reference stands on its own: for every position of the dense layer
    a float32 evaluation in natural k order and one in a random k order equal
    the float64 evaluation bit for bit (and `reference` checks its premises)."""
    feat = fx.inputs(96, n_in, seed=n_in + n_hidden)
    rng = np.random.default_rng(7)
    for d in range(n_hidden + 2):
        ws = fx.build(n_in, n_hidden, d, seed=d)
        assert [w.shape for w in ws] == [(64, n_in)] + [(64, 64)] * n_hidden + [(3, 64)]
        assert fx.dense_layer(ws) == d
        ref = fx.reference(ws, feat)
        assert np.array_equal(fx.forward_f32(ws, feat), ref), d
        assert np.array_equal(fx.forward_f32(ws, feat, rng), ref), d


@pytest.mark.parametrize("LF", [(16, 2), (8, 2), (21, 2), (1, 1)])
def test_encoder_case_features(oracle, LF):
    """The CPU encoder returns exactly the rows `encoder_case` expects in
    columns 0 : 3 + L F + 3 (p_norm, grid, wi)."""
    f = fx.make_field(LF[0], LF[1], 1, 0)
    p, wi, _, feat = fx.encoder_case(LF[0], LF[1], 200, seed=2)
    k = 3 + LF[0] * LF[1] + 3
    got = oracle.field_features(f, p, wi)
    assert np.array_equal(got[:, :k], feat[:, :k])
    assert (got[:, f.n_in:] == 0).all()


def test_encoder_fine_levels_are_hashed(oracle):
    """21 levels of a base-16, scale-2 grid: from level 18 on res^3 no longer
    fits 64 bits. Those levels must still be hashed (a wrapped res^3 once
    compared as "fits the table" and indexed them as dense). Lattice points
    and an integer table make the interpolation exact: the encoder's grid
    features equal sum(w * table[idx]) over `corners` (indices in Python
    integers)."""
    L, F = 21, 2
    f = fx.make_field(L, F, 0, 0)
    f.table[:] = np.random.default_rng(4).integers(0, 8, f.table.shape)
    p, wi, _, _ = fx.encoder_case(L, F, 100, seed=6)
    idx, w = fx.corners(f, p)
    lev = np.broadcast_to(np.arange(L)[None, :, None], idx.shape)
    want = (w.astype(np.float64)[..., None] * f.table[lev, idx].astype(np.float64)).sum(axis=2)
    assert np.array_equal(want * 512, np.round(want * 512))  # multiples of 1/512 below 8: exact in f32
    got = oracle.field_features(f, p, wi)[:, 3:3 + L * F]
    assert np.array_equal(got.reshape(len(p), L, F), want.astype(np.float16))  # one rounding, to fp16


# ------------------------------------------------------------------ GPU ----
def _mlp_field(n_levels, n_features, n_hidden, d, seed=0):
    from mtx.field import Field

    f = Field(bbox=fx.BBOX, n_levels=n_levels, n_features=n_features, n_hidden=n_hidden, log2_table=4)
    f.weights = fx.build(f.n_in, n_hidden, d, seed)
    return f


def _depth_cases():
    out = []
    for nh in (0, 1, 4, 14, 16):
        for d in sorted({0, 1, nh // 2, nh, nh + 1}):
            out.append((nh, d))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n_hidden,d", _depth_cases())
def test_mlp_depth_and_dense_position(n_hidden, d):
    f = _mlp_field(16, 2, n_hidden, d, seed=10 * n_hidden + d)
    feat = fx.inputs(200, f.n_in, seed=d)
    out = f.mlp(feat)
    assert np.array_equal(out, fx.reference(f.weights, feat))
    assert len(np.unique(out)) > 50


@pytest.mark.gpu
@pytest.mark.parametrize("LF,n_in", [((1, 1), 23), ((8, 2), 38), ((16, 1), 38), ((16, 2), 54), ((21, 2), 64)])
def test_mlp_input_width(LF, n_in):
    """Layer 0 with and without zero padding; what sits in the padding
    columns of a feature row must not matter (their weights are zero)."""
    f = _mlp_field(LF[0], LF[1], 1, 0, seed=n_in)
    assert f.n_in == n_in
    feat = fx.inputs(200, n_in, seed=3)
    ref = fx.reference(f.weights, feat)
    assert np.array_equal(f.mlp(feat), ref)
    if n_in < 64:
        assert np.array_equal(f.mlp(fx.inputs(200, n_in, seed=3, pad=7)), ref)


@pytest.mark.gpu
def test_mlp_tile_edges():
    """Query counts around the 32-query N-tile, the 64-query wave tile and
    the 256-query block."""
    f = _mlp_field(16, 2, 4, 2, seed=5)
    for n in (1, 31, 32, 33, 63, 64, 65, 255, 256, 257):
        feat = fx.inputs(n, f.n_in, seed=n)
        assert np.array_equal(f.mlp(feat), fx.reference(f.weights, feat)), n


@pytest.mark.gpu
def test_mlp_second_tile_per_wave():
    """More tiles than waves (the grid is capped at 3 blocks of 4 waves per
    CU): the `tile += n_waves` loop and its prefetch run, the last wave's
    second tile is partial. Every row is checked."""
    import torch

    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 64 * (12 * n_cu) + 65
    f = _mlp_field(16, 2, 4, 0, seed=8)
    feat = fx.inputs(n, f.n_in, seed=9)
    out = f.mlp(feat)
    ref = fx.reference(f.weights, feat)
    assert np.array_equal(out, ref), np.argwhere(out != ref)[:5]


@pytest.mark.gpu
@pytest.mark.parametrize("d", [0, 2])
def test_field_through_encoder(d):
    """Field.features and Field.__call__ (encoder + MLP in one call) on
    lattice queries: exact feature rows, then the radiance bit for bit."""
    L, F = 16, 2
    f = fx.make_field(L, F, 4, d, seed=3 + d)
    k = 3 + L * F + 3
    for n in (1, 65, 1000):
        p, wi, _, feat = fx.encoder_case(L, F, n, seed=n, signed_wi=d == 0)
        assert np.array_equal(f.features(p, wi)[:, :k], feat[:, :k]), n
        ref = fx.reference(f.weights, feat, frac_bits=3)
        assert np.array_equal(f(p, wi), ref), n
    assert len(np.unique(ref)) > 50


@pytest.mark.gpu
def test_encoder_fine_levels_device(oracle):
    """The device encoder on the 21-level grid of the CPU test above (the
    other encoder tests stop at 16 levels): bit for bit the CPU rows."""
    f = fx.make_field(21, 2, 0, 0)
    f.table[:] = np.random.default_rng(4).integers(0, 8, f.table.shape)
    p, wi, _, _ = fx.encoder_case(21, 2, 300, seed=6)
    assert np.array_equal(f.features(p, wi).view(np.uint16), oracle.field_features(f, p, wi).view(np.uint16))


# ---------------------------------------------------------------- training --
def _gscale_scale(n, g=1.0):
    """Loss scale for which dL/dout's factor 2 scale / (3 n) is the power of two g."""
    return 1.5 * n * g


def _check_training(oracle, f, p, wi, feat, target, scale):
    """mtx_field_grad against the float64 backward pass of the exact network.

    Forward: out equals the reference and Field.__call__ bit for bit; loss
    within 3n * 2^-24 relative. Gradients: the activations are exact, so the
    derivative masks of the device and the reference coincide and the only
    difference left is fp32 rounding: |g - g_ref| <= 4 K 2^-24 A per element,
    A the same sum over magnitudes, K the number of fp32 terms on the longest
    chain into that element (64 per dX layer above it, the 64 points of a
    block, the blocks; for a table entry all dX layers and the corners
    scattered to it); the factor 4 covers the f32 slope constant, the fp32
    gscale and the rounding of each product. Derived, not measured.

    The feature rows come from the CPU encoder: the network ignores the SH
    columns (zero weights), but layer 0's gradient there is dY X^T with the
    real SH values."""
    from mtx.nerad import field_grad

    n = len(p)
    k = 3 + f.n_levels * f.n_features + 3
    exact, feat = feat, oracle.field_features(f, p, wi)
    assert np.array_equal(feat[:, :k], exact[:, :k]) and (feat[:, f.n_in:] == 0).all()
    r = fx.backward(f.weights, feat, target, scale, frac_bits=3)
    loss, out, gt, gw = field_grad(f, p, wi, target, scale)
    assert np.array_equal(out, r["out"])
    assert np.array_equal(f(p, wi), r["out"])
    assert abs(loss - r["loss"]) <= 3 * n * EPS32 * r["loss"]
    n_layers, blocks = len(f.weights), (n + 63) // 64
    for l in range(n_layers):
        K = 64 * (n_layers - 1 - l) + 64 + blocks
        bound = 4 * K * EPS32 * r["aW"][l] + 1e-37
        err = np.abs(gw[l] - r["gW"][l])
        assert (err <= bound).all(), (l, np.argwhere(err > bound)[:5], (err / np.maximum(r["aW"][l], 1e-300)).max())
        assert np.abs(r["gW"][l]).max() > 0
    # table: d(grid features) scattered to the 8 corners of every level
    L, F = f.n_levels, f.n_features
    dgrid = r["dX"][:, 3:3 + L * F].reshape(n, L, F)
    agrid = r["aX"][:, 3:3 + L * F].reshape(n, L, F)
    idx, w = fx.corners(f, p)
    ref_t, a_t = np.zeros(gt.shape, np.float64), np.zeros(gt.shape, np.float64)
    hits = np.zeros(gt.shape[:2], np.int64)
    lev = np.broadcast_to(np.arange(L)[None, :, None], idx.shape)
    np.add.at(hits, (lev, idx), 1)
    for k in range(F):
        np.add.at(ref_t[..., k], (lev, idx), w.astype(np.float64) * dgrid[:, :, None, k])
        np.add.at(a_t[..., k], (lev, idx), w.astype(np.float64) * agrid[:, :, None, k])
    K = 64 * n_layers + int(hits.max())
    err = np.abs(gt - ref_t)
    bound = 4 * K * EPS32 * a_t + 1e-37
    assert (err <= bound).all(), (np.argwhere(err > bound)[:5], (err / np.maximum(a_t, 1e-300)).max())
    assert np.abs(ref_t).max() > 0
    # per level the entries sum to the level's d(grid features): the trilinear
    # weights of a point sum to one (8 more roundings)
    sbound = 4 * (K + 8) * EPS32 * agrid.sum(axis=0) + 1e-37
    assert (np.abs(gt.astype(np.float64).sum(axis=1) - dgrid.sum(axis=0)) <= sbound).all()
    return r, gt, gw


def _train_case(L, F, n_hidden, d, n, seed=0, distinct=False, zero_pnorm=False):
    """Field, lattice queries, their exact feature rows and targets that are
    multiples of 1/8. The grid features are the same for every query, so
    with the dense layer late the sign of a row barely varies over the batch:
    the first seed whose network keeps the reference's premises (both signs
    after layer d; decided on the CPU reference alone) is taken."""
    p, wi, _, feat = fx.encoder_case(L, F, n, seed=seed + 1, signed_wi=d == 0, distinct=distinct)
    target = np.random.default_rng(seed + 2).integers(-16, 17, (n, 3)).astype(np.float32) / 8
    for s in range(seed, seed + 64):
        f = fx.make_field(L, F, n_hidden, d, seed=s, zero_pnorm=zero_pnorm)
        try:
            fx.forward(f.weights, feat, frac_bits=3)
        except AssertionError:
            continue
        return f, p, wi, feat, target
    raise AssertionError("no seed keeps the premises of the exact network")


def _train_cases():
    cases = [(16, 2, nh, d, 192) for nh in (0, 1, 4, 13) for d in (0, nh + 1)] + [(16, 2, 4, 2, 192)]
    cases += [(16, 2, 4, 2, n) for n in (1, 63, 64, 65)]
    cases += [(16, 2, 1, 0, 65), (16, 2, 13, 14, 65), (16, 2, 0, 1, 1)]
    cases += [(8, 2, 1, 0, 192), (8, 2, 4, 5, 63), (21, 2, 1, 2, 192), (21, 2, 4, 0, 65)]
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("L,F,n_hidden,d,n", _train_cases())
def test_train_forward_and_gradients(oracle, L, F, n_hidden, d, n):
    f, p, wi, feat, target = _train_case(L, F, n_hidden, d, n, seed=n_hidden + d)
    _check_training(oracle, f, p, wi, feat, target, _gscale_scale(n, 4.0 if n in (63, 65) else 1.0))


@pytest.mark.gpu
def test_table_gradient_under_collisions(oracle):
    """50 distinct points, then the same batch three times (n = 150 spans
    three blocks and every corner is hit at least three times by the
    atomics). The loss is a mean: at equal gscale the second gradient is
    three times the first, each within its fp32 bound of the float64 one."""
    f, p, wi, feat, target = _train_case(16, 2, 4, 0, 50, seed=11, distinct=True)
    assert len(np.unique(p, axis=0)) == 50
    r1, gt1, gw1 = _check_training(oracle, f, p, wi, feat, target, _gscale_scale(50))
    rep = lambda a: np.tile(a, (3, 1))
    r3, gt3, gw3 = _check_training(oracle, f, rep(p), rep(wi), rep(feat), rep(target), _gscale_scale(150))
    assert abs(r3["loss"] - r1["loss"]) <= 1e-12 * r1["loss"]
    for a, b in zip(r3["gW"], r1["gW"]):  # the float64 gradients both runs were held to
        np.testing.assert_allclose(a, 3.0 * b, rtol=1e-12, atol=0)
    assert min(np.count_nonzero(gt1), np.count_nonzero(gt3)) > 8 * 16  # more than one point's corners


@pytest.mark.gpu
@pytest.mark.parametrize("n_hidden", [14, 16])
def test_deep_field_training(oracle, n_hidden):
    """Fields whose training tile (every layer's activations in LDS) exceeds
    a workgroup's LDS: mtx_field_grad either passes the exact checks or
    raises with the LDS requirement, on the host before anything is launched;
    field_train_init and field_train_step then raise as well, and the field
    on the device is unchanged (inference gives the same radiance)."""
    from mtx._lib import MtxError
    from mtx.nerad import field_grad, field_params, field_train_init, field_train_step

    f, p, wi, feat, target = _train_case(16, 2, n_hidden, 0, 192, seed=n_hidden, zero_pnorm=True)
    before = f(p, wi)
    assert np.array_equal(before, fx.reference(f.weights, feat, frac_bits=3))
    try:
        field_grad(f, p, wi, target, _gscale_scale(192))
    except MtxError as e:
        assert "LDS" in str(e) and str(n_hidden) in str(e), str(e)
    else:
        _check_training(oracle, f, p, wi, feat, target, _gscale_scale(192))
        return
    with pytest.raises(MtxError, match="LDS"):
        field_train_init(f)
    with pytest.raises(MtxError):
        field_train_step(f, p, wi, target)
    with pytest.raises(MtxError):  # training never started: there are no master copies
        field_params(f)
    assert np.array_equal(f(p, wi), before)
