"""An fp16 field network whose every pre-activation is exact, whatever order
the products are summed in (shared by tests/test_field_exact.py and
tests/test_nerad.py; a plain module, not a conftest).

The network has n_hidden + 2 layers (n_in -> 64, n_hidden x 64 -> 64,
64 -> 3), one of them dense, at position d:

* layers before d: a selection with weight 1, row o reads input
  (7 o + 3) mod in;
* layer d: dense, weights drawn from {-1, 0, 1};
* hidden layers after d: a permutation with weight -8, row o of layer l
  reads (5 o + 1 + l) mod 64;
* the output layer, when it is not the dense one: row r reads
  11 r + 2 + l with weights +1, -1, +1.

Inputs are integers 0..7. Up to layer d every value is a non-negative integer
and LeakyReLU is the identity. Layer d sums at most 64 integers of magnitude
<= 7: |sum| <= 448, exact in f32 and in fp16 in any order, both signs occur.
Every later layer is one product by +-2^k followed by max(h, h * fp16(0.01))
in fp16: one correctly rounded operation each, so no summation order is left.
The -8 negates every value at every layer, so a value takes the slope at
every other layer and never decays.

Through the encoder (`encoder_case`) the inputs are p_norm = k / 8, constant
integer grid features and an integer wi: multiples of 1/8, which the same
argument covers with `frac_bits = 3` (layer d's sums are then exact in fp16
below 256). A selection layer cannot pass a negative value on exactly (it
would take the slope before the dense layer and the sums of such values are
no longer order-free), so wi is signed only for d = 0.

`reference` asserts on every call that the input it was given keeps these
premises, so a test cannot pass on a network that exercises nothing.
"""
import numpy as np

SLOPE16 = np.float16(0.01)
F16_MIN_NORMAL = 2.0 ** -14
F16_MAX = 65504.0


def build(n_in, n_hidden, d, seed=0, zero_cols=()):
    """fp16 weight matrices [(64, n_in), n_hidden x (64, 64), (3, 64)] of the
    network above; `zero_cols`: layer-0 input columns whose weights are zero
    (features the construction does not control, e.g. the SH block)."""
    n_layers = n_hidden + 2
    assert 0 <= d < n_layers
    rng = np.random.default_rng(seed)
    ws = []
    for l in range(n_layers):
        cin = n_in if l == 0 else 64
        out = 3 if l == n_layers - 1 else 64
        w = np.zeros((out, cin), np.float16)
        if l == d:
            # as many +1 as -1 in every row: the inputs have mean 3.5, so an
            # unbalanced row (and with it one of only 3 output rows) would
            # lean to one sign for every query
            row = np.zeros(cin, np.float16)
            row[: cin // 3], row[cin // 3: 2 * (cin // 3)] = 1, -1
            for o in range(out):
                w[o] = rng.permutation(row)
        elif l < d:
            for o in range(out):
                w[o, (7 * o + 3) % cin] = 1
        elif l < n_layers - 1:
            for o in range(out):
                w[o, (5 * o + 1 + l) % 64] = -8
        else:
            for r, s in enumerate((1, -1, 1)):
                w[r, 11 * r + 2 + l] = s
        if l == 0 and len(zero_cols):
            w[:, list(zero_cols)] = 0
        ws.append(w)
    return ws


def inputs(n, n_in, seed=0, pad=0):
    """(n, 64) fp16 feature rows: integers 0..7 in the first n_in columns,
    `pad` in the padding columns (their layer-0 weights do not exist)."""
    rng = np.random.default_rng(seed)
    feat = np.full((n, 64), pad, np.float16)
    feat[:, :n_in] = rng.integers(0, 8, (n, n_in))
    return feat


def dense_layer(weights):
    """Position d of the dense layer: the only one with several weights per row."""
    for l, w in enumerate(weights):
        if (np.count_nonzero(w, axis=1) > 1).any():
            return l
    raise AssertionError("no dense layer in this network")


def forward(weights, feat, frac_bits=0):
    """float64 forward pass with fp16 rounding after every layer and
    LeakyReLU evaluated in numpy fp16 (as Field.mlp_reference): returns
    (acts, out) with acts[l] the float64 input of layer l and out the
    fp16-rounded output as float64. Asserts the premises of the module
    docstring."""
    d = dense_layer(weights)
    last = len(weights) - 1
    x = np.asarray(feat, np.float16).astype(np.float64)[:, : weights[0].shape[1]]
    acts, signs = [], []
    for l, w in enumerate(weights):
        acts.append(x)
        pre = x @ w.astype(np.float64).T
        if l == d:  # 1. exact in f32 (any order) and in fp16
            m = pre * 2.0 ** frac_bits
            assert np.array_equal(m, np.round(m)) and np.abs(m).max() < 2048, "layer d is not exact"
        h = pre.astype(np.float16)
        a = np.maximum(h, h * SLOPE16) if l < last else h
        v = np.abs(a.astype(np.float64))
        nz = v[v != 0]  # 2. fp16 normal range: no subnormal handling involved
        assert nz.size == 0 or (nz.min() >= F16_MIN_NORMAL and nz.max() < F16_MAX), "activation out of range"
        if l >= d:
            signs.append(np.sign(h.astype(np.float64)).reshape(-1))
        x = a.astype(np.float64)
    s = np.concatenate(signs)  # 3. both branches of LeakyReLU taken after layer d
    assert (s < 0).mean() >= 0.25 and (s > 0).mean() >= 0.25, ((s < 0).mean(), (s > 0).mean())
    return acts, x


def reference(weights, feat, frac_bits=0):
    """The network's output (n, 3) as float64 (exactly fp16 values)."""
    return forward(weights, feat, frac_bits)[1]


def forward_f32(weights, feat, order_rng=None):
    """The same network with every layer accumulated in float32, one k at a
    time, in natural order or in the random orders drawn from `order_rng`
    (a different one per layer): what a device sum in some order computes."""
    last = len(weights) - 1
    x = np.asarray(feat, np.float16).astype(np.float32)[:, : weights[0].shape[1]]
    for l, w in enumerate(weights):
        w32 = w.astype(np.float32)
        order = np.arange(w.shape[1]) if order_rng is None else order_rng.permutation(w.shape[1])
        acc = np.zeros((len(x), w.shape[0]), np.float32)
        for k in order:
            acc = acc + x[:, k:k + 1] * w32[None, :, k]
        h = acc.astype(np.float16)
        x = (np.maximum(h, h * SLOPE16) if l < last else h).astype(np.float32)
    return x


def backward(weights, feat, target, scale, frac_bits=0):
    """float64 backward pass of scale * mean((out - target)^2) through the
    network above. Returns a dict with loss, out, the weight gradients gW[l],
    the gradient dX w.r.t. the input features (n, n_in), and aW / aX: the same
    sums with |dY|, |W|, |X| and the slope factors in place of the signed
    quantities (the magnitude every fp32 rounding error is relative to)."""
    acts, out = forward(weights, feat, frac_bits)
    Ws = [w.astype(np.float64) for w in weights]
    n = len(out)
    diff = out - np.asarray(target, np.float64)
    dY = scale * 2.0 * diff / (3.0 * n)
    aY = np.abs(dY)
    gW, aW = [None] * len(Ws), [None] * len(Ws)
    for l in range(len(Ws) - 1, -1, -1):
        if l < len(Ws) - 1:
            s = np.where(acts[l + 1] > 0, 1.0, 0.01)
            dY, aY = dY * s, aY * s
        gW[l] = dY.T @ acts[l]
        aW[l] = aY.T @ np.abs(acts[l])
        dY, aY = dY @ Ws[l], aY @ np.abs(Ws[l])
    return {"loss": float((diff * diff).mean()), "out": out, "gW": gW, "aW": aW, "dX": dY, "aX": aY}


# ------------------------------------------------------- through the encoder --
BBOX = ([0.0, 0.0, 0.0], [8.0, 8.0, 8.0])


def table_constants(n_levels, n_features):
    """table[l, :, f]: one small integer (1..7) per (level, feature)."""
    l, f = np.meshgrid(np.arange(n_levels), np.arange(n_features), indexing="ij")
    return ((3 * l + 5 * f) % 7 + 1).astype(np.float16)


def encoder_case(n_levels, n_features, n, seed=0, signed_wi=True, distinct=False):
    """Queries whose feature rows are exact: p on the lattice {1..7}^3 of the
    box [0, 8]^3 (p_norm = k / 8), wi a small integer vector (the encoder
    passes wi through unnormalised), a table that is constant per (level,
    feature). Returns p, wi, the constants and the expected feature rows
    (n, 64) with the 16 SH columns and the padding left at zero: the networks
    used with it carry zero weights there (`sh_cols`)."""
    rng = np.random.default_rng(seed)
    if distinct:
        assert n <= 343
        k = rng.permutation(343)[:n]
        p = np.stack([k % 7, (k // 7) % 7, k // 49], axis=1) + 1
    else:
        p = rng.integers(1, 8, (n, 3))
    wi = rng.integers(-3, 4, (n, 3)) if signed_wi else rng.integers(0, 4, (n, 3))
    c = table_constants(n_levels, n_features)
    LF = n_levels * n_features
    feat = np.zeros((n, 64), np.float16)
    feat[:, 0:3] = p / 8.0
    feat[:, 3:3 + LF] = c.reshape(-1)
    feat[:, 3 + LF:6 + LF] = wi
    return p.astype(np.float32), wi.astype(np.float32), c, feat


def sh_cols(n_levels, n_features):
    k = 3 + n_levels * n_features + 3
    return range(k, k + 16)


def make_field(n_levels, n_features, n_hidden, d, seed=0, log2_table=12, zero_pnorm=False):
    """A Field on BBOX with the constant table and the exact network (zero
    weights on the SH columns), set before its first upload. `zero_pnorm`
    also zeroes the weights of the three p_norm columns: the inputs are then
    integers, which the deepest networks need (a value of 1/8 decays below
    fp16's normal range after 16 slope layers)."""
    from mtx.field import Field

    f = Field(bbox=BBOX, n_levels=n_levels, n_features=n_features, n_hidden=n_hidden, log2_table=log2_table)
    f.table[:] = table_constants(n_levels, n_features)[:, None, :]
    zero = list(sh_cols(n_levels, n_features)) + ([0, 1, 2] if zero_pnorm else [])
    f.weights = build(f.n_in, n_hidden, d, seed, zero_cols=zero)
    return f


def corners(field, p):
    """Per level the 8 table indices and trilinear weights of every point
    (mtx_core/field.h field_level_corners in float32, the fused multiply-add
    through float64): idx (n, L, 8) int64, w (n, L, 8) float32."""
    f32 = np.float32
    span = (field.bbox_max - field.bbox_min).astype(f32)
    pn = ((np.asarray(p, f32) - field.bbox_min) / span).astype(f32)
    T = 1 << field.log2_table
    n, L = len(pn), field.n_levels
    idx = np.zeros((n, L, 8), np.int64)
    w = np.zeros((n, L, 8), f32)
    for l in range(L):
        scale = f32(np.exp2(l * np.log2(field.per_level_scale)) * field.base_res - 1.0)
        res = int(np.ceil(float(scale))) + 1
        dense = res ** 3 <= T
        pos = (pn.astype(np.float64) * np.float64(scale) + 0.5).astype(f32)  # fmaf: one rounding
        g = np.floor(pos)
        t = (pos - g).astype(f32)
        g = g.astype(np.int64)
        for c in range(8):
            b = np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1])
            x, y, z = ((g + b) & 0xFFFFFFFF).T
            if dense:
                i = x + y * res + z * res * res
            else:
                i = x ^ ((y * 2654435761) & 0xFFFFFFFF) ^ ((z * 805459861) & 0xFFFFFFFF)
            idx[:, l, c] = i & (T - 1)
            ww = np.ones(n, f32)
            for k in range(3):
                ww = (ww * (t[:, k] if b[k] else f32(1) - t[:, k])).astype(f32)
            w[:, l, c] = ww
    return idx, w
