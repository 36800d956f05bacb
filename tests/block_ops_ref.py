"""Float64 references of the block message-passing ops (csrc/block_ops.hip) and a priori
bounds on the error of their fp32 kernels, plus the seeded inputs that the CPU and GPU tests
of those ops share.  Pure numpy: imports and runs without a GPU.

Every reference takes the block as given -- `col` (source index per edge), `row`
(destination index per edge), `num_dst`, `num_src` -- and no layout is assumed, so a block
whose col-less fast path relies on a broken invariant shows up as a mismatch.

Error bounds.  u = 2^-24 and gamma_k = k u / (1 - k u).  The library is built with
-ffp-contract=off and without fast-math, so every fp32 add and multiply is one correctly
rounded operation and the standard bounds hold for any summation order (serial, lane-strided
or a shuffle tree).  Each bound also carries a float64 slack of 4 n 2^-53 sum|terms| for the
reference's own rounding.  A CPU emulation of the kernels' algorithms (v_exp_f32 perturbed
by +-1 ulp) stays well inside these bounds; see tests/test_block_ops_ref.py.
"""
import numpy as np

U = 2.0 ** -24              # unit roundoff of fp32
U64 = 2.0 ** -53            # unit roundoff of float64
TINY = 2.0 ** -126          # smallest normal fp32: results that flush to zero


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def _slack(n):
    return 4.0 * np.asarray(n, dtype=np.float64) * U64


# ---- layout -------------------------------------------------------------------------------
def _layout(col, row, num_dst, num_src):
    col = np.asarray(col, dtype=np.int64).reshape(-1)
    row = np.asarray(row, dtype=np.int64).reshape(-1)
    if col.shape != row.shape:
        raise ValueError("col and row differ in length")
    if len(row) and (row.min() < 0 or row.max() >= num_dst):
        raise ValueError("row index outside [0, num_dst)")
    if len(col) and (col.min() < 0 or col.max() >= num_src):
        raise ValueError("col index outside [0, num_src)")
    return col, row


def _scatter(ufunc, index, values, n, fill):
    """out[i] = ufunc over values[index == i] (`fill` where there is none); any index order."""
    out = np.full((n,) + values.shape[1:], fill, dtype=values.dtype)
    if len(index) == 0:
        return out
    order = np.argsort(index, kind="stable")
    idx = index[order]
    starts = np.flatnonzero(np.r_[True, idx[1:] != idx[:-1]])
    out[idx[starts]] = ufunc.reduceat(values[order], starts, axis=0)
    return out


def degrees(row, num_dst):
    return np.bincount(np.asarray(row, dtype=np.int64), minlength=num_dst)[:num_dst]


def _rows(a, n):
    """[n, ...] -> [n, prod(...)] in float64 (also for n = 0)."""
    a = np.asarray(a, dtype=np.float64)
    return a.reshape(n, int(np.prod(a.shape[1:])))


def _weights(w, E, dim):
    """[E, heads(, 1)] edge weights -> (w [E, H], column c's head = c // (dim / H))."""
    w = _rows(w, E)
    H = w.shape[1]
    if dim % H:
        raise ValueError("feature size is not a multiple of the heads")
    return w, np.arange(dim) // (dim // H)


def _mean_scale(n, mean):
    n = np.asarray(n, dtype=np.float64)
    return np.where(mean & (n > 0), 1.0 / np.maximum(n, 1.0), 1.0)


# ---- block_reduce: out[d] = scale_d * sum_{k into d} w[k, head(c)] * src[col[k], c] -------
def reduce_fwd(col, row, num_dst, num_src, src, w=None, mean=False):
    col, row = _layout(col, row, num_dst, num_src)
    src = _rows(src, num_src)
    msg = src[col]
    if w is not None:
        w, head = _weights(w, len(col), src.shape[1])
        msg = msg * w[:, head]
    out = _scatter(np.add, row, msg, num_dst, 0.0)
    return out * _mean_scale(degrees(row, num_dst), mean)[:, None]


def reduce_fwd_bound(col, row, num_dst, num_src, src, w=None, mean=False):
    """gamma_{n+3} scale sum_k |w_k v_k| over the n edges of the segment: n products, n - 1
    adds, and for mean the rounding of 1/n and of its multiply."""
    col, row = _layout(col, row, num_dst, num_src)
    src = _rows(src, num_src)
    msg = np.abs(src[col])
    if w is not None:
        w, head = _weights(w, len(col), src.shape[1])
        msg = msg * np.abs(w[:, head])
    n = degrees(row, num_dst)
    total = _scatter(np.add, row, msg, num_dst, 0.0) * _mean_scale(n, mean)[:, None]
    return (gamma(n + 3) + _slack(n))[:, None] * total


def reduce_bwd(col, row, num_dst, num_src, src, w, mean, grad_out):
    """(grad_src [num_src, dim], grad_w [E, H] or None)."""
    col, row = _layout(col, row, num_dst, num_src)
    src = _rows(src, num_src)
    g = _rows(grad_out, num_dst)
    ge = g[row] * _mean_scale(degrees(row, num_dst), mean)[row][:, None]
    grad_w = None
    if w is not None:
        w, head = _weights(w, len(col), src.shape[1])
        H = w.shape[1]
        grad_w = (ge * src[col]).reshape(len(col), H, src.shape[1] // H).sum(-1)
        ge = ge * w[:, head]
    return _scatter(np.add, col, ge, num_src, 0.0), grad_w


def reduce_bwd_bound(col, row, num_dst, num_src, src, w, mean, grad_out):
    """grad_src: gamma_{m+3} sum |g scale w| over the m edges that read the row (m = 1 in the
    sampler's layout; rows no edge reads must be exactly 0).  grad_w: gamma_{p+2} scale
    sum_c |g v| over the head's p = dim / heads columns."""
    col, row = _layout(col, row, num_dst, num_src)
    src = _rows(src, num_src)
    g = _rows(grad_out, num_dst)
    ge = np.abs(g[row]) * _mean_scale(degrees(row, num_dst), mean)[row][:, None]
    bound_w = None
    if w is not None:
        w, head = _weights(w, len(col), src.shape[1])
        H = w.shape[1]
        p = src.shape[1] // H
        bound_w = (gamma(p + 2) + _slack(p)) * \
            (ge * np.abs(src[col])).reshape(len(col), H, src.shape[1] // H).sum(-1)
        ge = ge * np.abs(w[:, head])
    m = np.bincount(col, minlength=num_src)[:num_src]
    bound_src = (gamma(m + 3) + _slack(m))[:, None] * _scatter(np.add, col, ge, num_src, 0.0)
    return bound_src, bound_w


# ---- edge_softmax over the edges that share a destination -------------------------------------
def _softmax_max(row, num_dst, x):
    return _scatter(np.maximum, row, x, num_dst, -np.inf)


def softmax_fwd(col, row, num_dst, num_src, x):
    """x [E, H]; a segment whose logits are all -inf gives NaN (as dgl)."""
    col, row = _layout(col, row, num_dst, num_src)
    x = _rows(x, len(row))
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.exp(x - _softmax_max(row, num_dst, x)[row])
        return e / _scatter(np.add, row, e, num_dst, 0.0)[row]


def softmax_fwd_bound(col, row, num_dst, num_src, x):
    """|y_k| (t_k + sum_j y_j t_j + (n + 1) u) + 2^-126, t_k = u (3 |x_k - m| + 2).

    __expf(z) is v_exp_f32(log2e * z): the rounding of x - m and of the multiply perturb the
    exponent by about 3 u |x - m|, v_exp_f32 is taken as accurate to 1 ulp (its ISA
    specification; the +2), the sum of the n terms and 1 / s add (n + 1) u.  The absolute
    2^-126 covers terms that flush to zero.  Masked (-inf) logits contribute nothing; they
    must come out exactly 0, which the caller checks."""
    col, row = _layout(col, row, num_dst, num_src)
    x = _rows(x, len(row))
    y = softmax_fwd(col, row, num_dst, num_src, x)
    with np.errstate(invalid="ignore"):
        a = np.abs(x - _softmax_max(row, num_dst, x)[row])
    live = np.isfinite(a)
    t = np.where(live, U * (3.0 * np.where(live, a, 0.0) + 2.0), 0.0)
    yt = np.where(live, np.nan_to_num(y) * t, 0.0)
    n = degrees(row, num_dst)[row][:, None]
    rel = t + _scatter(np.add, row, yt, num_dst, 0.0)[row] + (n + 1) * U + _slack(n)
    return np.abs(y) * rel + TINY


def softmax_bwd(col, row, num_dst, num_src, y, grad_y):
    """grad_x = y (grad_y - sum_segment(grad_y y)), from the given (kernel's own) y."""
    col, row = _layout(col, row, num_dst, num_src)
    y, gy = _rows(y, len(row)), _rows(grad_y, len(row))
    dot = _scatter(np.add, row, gy * y, num_dst, 0.0)
    return y * (gy - dot[row])


def softmax_bwd_bound(col, row, num_dst, num_src, y, grad_y):
    """|y_k| (gamma_{n+2} sum_j |gy_j y_j| + gamma_2 |gy_k - dot|)."""
    col, row = _layout(col, row, num_dst, num_src)
    y, gy = _rows(y, len(row)), _rows(grad_y, len(row))
    dot = _scatter(np.add, row, gy * y, num_dst, 0.0)
    n = degrees(row, num_dst)[row][:, None]
    a = _scatter(np.add, row, np.abs(gy * y), num_dst, 0.0)[row]
    return np.abs(y) * ((gamma(n + 2) + _slack(n)) * a + gamma(2) * np.abs(gy - dot[row]))


# ---- block_max: out[d, c] = max over the edges into d (0 without any) ----------------------------
def max_fwd(col, row, num_dst, num_src, src):
    """(out [num_dst, dim], arg [num_dst, dim]): arg is the winning edge, the LOWEST edge
    index in segment order on ties (the stable grouping of edges by destination), -1 for a
    destination without in-edges."""
    col, row = _layout(col, row, num_dst, num_src)
    src = _rows(src, num_src)
    E, dim = len(col), src.shape[1]
    v = src[col]
    best = _scatter(np.maximum, row, v, num_dst, -np.inf)
    order = np.argsort(row, kind="stable")          # segment order
    pos = np.empty(E, dtype=np.int64)
    pos[order] = np.arange(E)
    cand = np.where(v == best[row], pos[:, None], E)
    first = _scatter(np.minimum, row, cand, num_dst, E)
    has = first < E
    arg = np.full(first.shape, -1, dtype=np.int64)
    arg[has] = order[first[has]]
    out = np.where(has, best, 0.0)
    return out.reshape(num_dst, dim), arg.reshape(num_dst, dim)


def max_bwd(col, row, num_dst, num_src, arg, grad_out):
    """grad_src[col[arg[d, c]], c] += grad_out[d, c]."""
    col, row = _layout(col, row, num_dst, num_src)
    g = _rows(grad_out, num_dst)
    arg = np.asarray(arg, dtype=np.int64).reshape(g.shape)
    dim = g.shape[1]
    out = np.zeros((num_src, dim))
    d, c = np.nonzero(arg >= 0)
    np.add.at(out, (col[arg[d, c]], c), g[d, c])
    return out


def max_bwd_bound(col, row, num_dst, num_src, arg, grad_out):
    """0 where a (source row, column) receives at most one value (always so in the sampler's
    layout); else gamma_m sum |g| over the m values it receives."""
    col, row = _layout(col, row, num_dst, num_src)
    g = _rows(grad_out, num_dst)
    arg = np.asarray(arg, dtype=np.int64).reshape(g.shape)
    dim = g.shape[1]
    a, m = np.zeros((num_src, dim)), np.zeros((num_src, dim))
    d, c = np.nonzero(arg >= 0)
    np.add.at(a, (col[arg[d, c]], c), np.abs(g[d, c]))
    np.add.at(m, (col[arg[d, c]], c), 1.0)
    return np.where(m >= 2, gamma(m) + _slack(m), 0.0) * a


# ---- comparison -----------------------------------------------------------------------------
def error_ratio(got, want, bound):
    """max |got - want| / bound, elementwise; inf where an error meets a zero bound or where the
    NaN pattern differs (NaN is expected exactly where the reference gives NaN)."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), want.shape)
    if got.shape != want.shape:
        raise ValueError("shape {} != {}".format(got.shape, want.shape))
    nan = np.isnan(want)
    if not np.array_equal(np.isnan(got), nan):
        return float("inf")
    if not nan.any() and got.size == 0:
        return 0.0
    err = np.abs(got - want)[~nan]
    b = bound[~nan]
    if (err > 0)[b == 0].any() or not np.isfinite(err).all():
        return float("inf")
    r = err[b > 0] / b[b > 0]
    return float(r.max()) if r.size else 0.0


# ---- seeded inputs shared by the CPU and the GPU tests ---------------------------------------
def block_layout(degs, sampler_layout, seed):
    """(col, row, num_dst, num_src) with edges grouped by destination.  sampler_layout: the
    sampler's col = num_dst + arange(E), num_src = num_dst + E; else sources drawn from a
    smaller pool so that a row feeds several edges (the explicit-col, atomic path)."""
    degs = np.asarray(degs, dtype=np.int64)
    num_dst = len(degs)
    row = np.repeat(np.arange(num_dst), degs).astype(np.int64)
    E = len(row)
    if sampler_layout:
        return num_dst + np.arange(E, dtype=np.int64), row, num_dst, num_dst + E
    rng = np.random.RandomState(seed)
    num_src = num_dst + max(E // 3, 1)
    return rng.randint(0, num_src, E).astype(np.int64), row, num_dst, num_src


def hand_degrees(num_dst, maxdeg, seed):
    """Degrees 0..maxdeg with zero-degree destinations first and last."""
    degs = np.random.RandomState(seed).randint(0, maxdeg + 1, num_dst)
    if num_dst > 2:
        degs[0] = degs[-1] = 0
    return degs


def width_case(dim, sampler_layout):
    """A sampled-layer-shaped block (degrees 0-10) with `dim` feature columns."""
    col, row, nd, ns = block_layout(hand_degrees(150, 10, 100 + dim), sampler_layout, 7)
    rng = np.random.RandomState(200 + dim)
    return dict(col=col, row=row, num_dst=nd, num_src=ns,
                src=rng.randn(ns, dim).astype(np.float32),
                w=rng.randn(len(col), 1).astype(np.float32),
                grad=rng.randn(nd, dim).astype(np.float32))


def head_case(per_head, heads, sampler_layout):
    """[E, H] edge weights over [num_src, H, per_head] features, and [E, H] logits."""
    col, row, nd, ns = block_layout(hand_degrees(90, 10, 300 + per_head + heads),
                                    sampler_layout, 8)
    rng = np.random.RandomState(400 + 10 * per_head + heads)
    E = len(col)
    return dict(col=col, row=row, num_dst=nd, num_src=ns,
                src=rng.randn(ns, heads, per_head).astype(np.float32),
                w=rng.randn(E, heads).astype(np.float32),
                grad=rng.randn(nd, heads, per_head).astype(np.float32),
                logits=(3 * rng.randn(E, heads)).astype(np.float32),
                grad_y=rng.randn(E, heads).astype(np.float32))


def softmax_switch_case(extra, heads):
    """num_dst = 64 and E = 32 num_dst + extra: extra = 0 stays on the thread kernels,
    extra = 1 is the smallest block that takes the wave kernels."""
    nd = 64
    rng = np.random.RandomState(500 + extra + 7 * heads)
    degs = rng.multinomial(32 * nd + extra, np.full(nd, 1.0 / nd))
    col, row, nd, ns = block_layout(degs, True, 0)
    E = len(col)
    return dict(col=col, row=row, num_dst=nd, num_src=ns,
                logits=(3 * rng.randn(E, heads)).astype(np.float32),
                grad_y=rng.randn(E, heads).astype(np.float32))


def long_segment_case(sampler_layout):
    """One destination with 3000 in-edges among 1000 of degree 0-3: still the thread path."""
    degs = hand_degrees(1000, 3, 600)
    degs[517] = 3000
    col, row, nd, ns = block_layout(degs, sampler_layout, 9)
    rng = np.random.RandomState(601)
    E, H, P = len(col), 2, 40
    return dict(col=col, row=row, num_dst=nd, num_src=ns,
                src=rng.randn(ns, H, P).astype(np.float32),
                w=rng.randn(E, H).astype(np.float32),
                grad=rng.randn(nd, H, P).astype(np.float32),
                logits=(3 * rng.randn(E, H)).astype(np.float32),
                grad_y=rng.randn(E, H).astype(np.float32))


def tie_case(sampler_layout):
    """Integer features in {0, 1, 2}, degrees 0-10: most outputs with two or more in-edges
    are ties, so the lowest-edge rule decides where their gradient goes."""
    col, row, nd, ns = block_layout(hand_degrees(400, 10, 700), sampler_layout, 10)
    rng = np.random.RandomState(701)
    D = 32
    return dict(col=col, row=row, num_dst=nd, num_src=ns,
                src=rng.randint(0, 3, (ns, D)).astype(np.float32),
                grad=rng.randn(nd, D).astype(np.float32))


def tie_fraction(col, row, num_dst, num_src, src):
    """Share of the (destination, column) outputs with >= 2 in-edges whose max is tied."""
    col, row = _layout(col, row, num_dst, num_src)
    src = _rows(src, num_src)
    best = _scatter(np.maximum, row, src[col], num_dst, -np.inf)
    hits = _scatter(np.add, row, (src[col] == best[row]).astype(np.float64), num_dst, 0.0)
    multi = degrees(row, num_dst) >= 2
    return float((hits[multi] >= 2).mean()) if multi.any() else 0.0


def softmax_edge_case(kind, wave):
    """Logits shifted per destination by up to +-1e4 ('shift'), with some -inf in every
    segment of two or more edges ('masked'), or with whole segments at -inf ('all_masked').
    wave: degrees 33-60 (the wave kernels) instead of 0-10 (the thread kernels)."""
    rng = np.random.RandomState(800 + 2 * ["shift", "masked", "all_masked"].index(kind) + wave)
    nd = 120
    degs = rng.randint(33, 61, nd) if wave else rng.randint(0, 11, nd)
    degs[0] = degs[-1] = 0
    col, row, nd, ns = block_layout(degs, True, 0)
    E, H = len(col), 3
    x = 3 * rng.randn(E, H)
    x += rng.uniform(-1e4, 1e4, (nd, 1))[row]
    if kind == "masked":
        starts = np.r_[0, np.cumsum(degs)[:-1]]
        for d in np.flatnonzero(degs >= 2):
            k = starts[d] + rng.choice(degs[d], rng.randint(1, degs[d]), replace=False)
            x[k, rng.randint(0, H)] = -np.inf
    elif kind == "all_masked":
        for d in np.flatnonzero(degs)[::4]:
            x[row == d, rng.randint(0, H)] = -np.inf
    return dict(col=col, row=row, num_dst=nd, num_src=ns, logits=x.astype(np.float32),
                grad_y=rng.randn(E, H).astype(np.float32))
