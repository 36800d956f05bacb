"""The float64 references and error bounds of tests/block_ops_ref.py, checked on the CPU before
any GPU run: an fp32 emulation of each kernel's algorithm (csrc/block_ops.hip) stays within
its bound, and seeded mistakes in that algorithm break it on the inputs that
tests/test_gpu_block_ops_fp64.py feeds the kernels -- so the bounds are neither wrong nor
vacuous."""
import numpy as np
import pytest

from tests import block_ops_ref as R

F32 = np.float32
LOG2E = F32(1.4426950408889634)       # the constant of clang's __expf


# ---- fp32 emulation of the kernels ------------------------------------------------------------
def _segment_table(row, num_dst):
    """[num_dst, maxdeg] edge indices in segment order (-1 past the segment), degrees."""
    row = np.asarray(row, dtype=np.int64)
    degs = R.degrees(row, num_dst)
    order = np.argsort(row, kind="stable")
    starts = np.r_[0, np.cumsum(degs)[:-1]]
    width = int(degs.max()) if len(degs) and len(row) else 0
    j = np.arange(width)
    table = np.where(j < degs[:, None], order[np.minimum(starts[:, None] + j, max(len(row) - 1, 0))]
                     if len(row) else -1, -1)
    return table, degs


def _heads_of(dim, heads, head_mod):
    per_head = dim // heads
    c = np.arange(dim)
    return c % heads if head_mod else c // per_head


def emu_reduce_fwd(c, mean, weighted, drop_last=False, mean_plus_one=False, head_mod=False):
    """segment_reduce_fwd: serial fp32 sum per (destination, column), then * (1 / n)."""
    col, row, nd, ns = c["col"], c["row"], c["num_dst"], c["num_src"]
    src = c["src"].reshape(ns, -1)
    dim = src.shape[1]
    table, degs = _segment_table(row, nd)
    w = c["w"].reshape(len(col), -1) if weighted else None
    acc = np.zeros((nd, dim), F32)
    for j in range(table.shape[1]):
        live = j < (degs - 1 if drop_last else degs)
        k = table[live, j]
        v = src[col[k]]
        if w is not None:
            v = v * w[k][:, _heads_of(dim, w.shape[1], head_mod)]
        acc[live] = acc[live] + v
    n = degs + 1 if mean_plus_one else degs
    scale = np.where(mean & (degs > 0), F32(1) / np.maximum(n, 1).astype(F32), F32(1))
    return acc * scale.astype(F32)[:, None]


def emu_reduce_bwd(c, mean, weighted, head_mod=False):
    """segment_reduce_bwd: g * scale * w[k, head] into grad_src (serial adds in edge order on
    a row read by several edges); grad_w = serial fp32 sum over the head's columns * scale."""
    col, row, nd, ns = c["col"], c["row"], c["num_dst"], c["num_src"]
    src = c["src"].reshape(ns, -1)
    g = c["grad"].reshape(nd, -1)
    dim = src.shape[1]
    degs = R.degrees(row, nd)
    scale = np.where(mean & (degs > 0), F32(1) / np.maximum(degs, 1).astype(F32), F32(1))
    ge = g[row] * scale.astype(F32)[row][:, None]
    gw = None
    if weighted:
        w = c["w"].reshape(len(col), -1)
        H = w.shape[1]
        p = dim // H
        gw = np.zeros((len(col), H), F32)
        for h in range(H):
            acc = np.zeros(len(col), F32)
            for cc in range(h * p, (h + 1) * p):
                acc = acc + g[row, cc] * src[col, cc]
            gw[:, h] = acc * scale.astype(F32)[row]
        ge = ge * w[:, _heads_of(dim, H, head_mod)]
    gs = np.zeros((ns, dim), F32)
    for k in range(len(col)):
        gs[col[k]] = gs[col[k]] + ge[k]
    return gs, gw


def _exp_f32(z, rng):
    """__expf(z) = v_exp_f32(log2e * z) in fp32, v_exp_f32 off by up to one ulp either way."""
    with np.errstate(invalid="ignore", over="ignore"):
        t = (z.astype(F32) * LOG2E).astype(F32)
        e = np.exp2(t.astype(np.float64)).astype(F32)
    step = np.where(e >= np.finfo(F32).tiny, rng.randint(-1, 2, e.shape), 0)   # 0 stays 0
    e = np.where(step > 0, np.nextafter(e, F32(np.inf)), e)
    return np.where(step < 0, np.nextafter(e, F32(0)), e).astype(F32)


def emu_softmax_fwd(c, seed=0, short_sum=False):
    """edge_softmax_fwd_*: m = max (from -FLT_MAX), s = serial sum of __expf(x - m),
    y = __expf(x - m) * (1 / s)."""
    row, nd = c["row"], c["num_dst"]
    x = c["logits"].reshape(len(row), -1).astype(F32)
    table, degs = _segment_table(row, nd)
    H = x.shape[1]
    m = np.full((nd, H), -np.finfo(F32).max, F32)
    for j in range(table.shape[1]):
        live = j < degs
        m[live] = np.fmax(m[live], x[table[live, j]])
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = _exp_f32((x - m[row]).astype(F32), np.random.RandomState(seed))
        s = np.zeros((nd, H), F32)
        for j in range(table.shape[1]):
            live = j < (degs - 1 if short_sum else degs)
            s[live] = s[live] + e[table[live, j]]
        inv = (F32(1) / s).astype(F32)
        return (e * inv[row]).astype(F32)


def emu_softmax_bwd(c, y):
    row, nd = c["row"], c["num_dst"]
    gy = c["grad_y"].reshape(len(row), -1).astype(F32)
    table, degs = _segment_table(row, nd)
    dot = np.zeros((nd, gy.shape[1]), F32)
    for j in range(table.shape[1]):
        live = j < degs
        k = table[live, j]
        dot[live] = dot[live] + gy[k] * y[k]
    return (y * (gy - dot[row])).astype(F32)


def emu_max(c, ties_to_highest=False):
    """segment_max_fwd + segment_max_bwd: serial scan with `v > best` (`>=` when mutated)."""
    col, row, nd, ns = c["col"], c["row"], c["num_dst"], c["num_src"]
    src = c["src"].reshape(ns, -1)
    g = c["grad"].reshape(nd, -1)
    table, degs = _segment_table(row, nd)
    best = np.zeros((nd, src.shape[1]), F32)
    who = np.full(best.shape, -1, np.int64)
    for j in range(table.shape[1]):
        live = j < degs
        k = table[live, j]
        v = src[col[k]]
        cur_b, cur_w = best[live], who[live]
        win = (cur_w < 0) | ((v >= cur_b) if ties_to_highest else (v > cur_b))
        best[live] = np.where(win, v, cur_b)
        who[live] = np.where(win, k[:, None], cur_w)
    gs = np.zeros((ns, src.shape[1]), F32)
    d, cc = np.nonzero(who >= 0)
    for i in range(len(d)):
        gs[col[who[d[i], cc[i]]], cc[i]] += g[d[i], cc[i]]
    return best, gs


# ---- the inputs of the GPU tests ----------------------------------------------------------------
REDUCE_CASES = [("width64_sampler", lambda: R.width_case(64, True)),
                ("width65_general", lambda: R.width_case(65, False)),
                ("width172_sampler", lambda: R.width_case(172, True)),
                ("head65x3_sampler", lambda: R.head_case(65, 3, True)),
                ("head1x8_general", lambda: R.head_case(1, 8, False)),
                ("long_segment", lambda: R.long_segment_case(True))]
SOFTMAX_CASES = [("switch_thread", lambda: R.softmax_switch_case(0, 4)),
                 ("switch_wave", lambda: R.softmax_switch_case(1, 4)),
                 ("head64x3", lambda: R.head_case(64, 3, True)),
                 ("long_segment", lambda: R.long_segment_case(True)),
                 ("shift_thread", lambda: R.softmax_edge_case("shift", False)),
                 ("shift_wave", lambda: R.softmax_edge_case("shift", True)),
                 ("masked_wave", lambda: R.softmax_edge_case("masked", True))]


def _ratio_fwd(c, mean, weighted, **mistake):
    w = c["w"] if weighted else None
    args = (c["col"], c["row"], c["num_dst"], c["num_src"], c["src"], w, mean)
    got = emu_reduce_fwd(c, mean, weighted, **mistake)
    return R.error_ratio(got, R.reduce_fwd(*args), R.reduce_fwd_bound(*args))


@pytest.mark.parametrize("name,make", REDUCE_CASES, ids=[n for n, _ in REDUCE_CASES])
@pytest.mark.parametrize("mode", ["copy_sum", "copy_mean", "mul_sum", "mul_mean"])
def test_reduce_emulation_within_bound(name, make, mode):
    c = make()
    mean, weighted = mode.endswith("mean"), mode.startswith("mul")
    assert _ratio_fwd(c, mean, weighted) <= 1.0
    w = c["w"] if weighted else None
    args = (c["col"], c["row"], c["num_dst"], c["num_src"], c["src"], w, mean, c["grad"])
    gs, gw = emu_reduce_bwd(c, mean, weighted)
    want_s, want_w = R.reduce_bwd(*args)
    bound_s, bound_w = R.reduce_bwd_bound(*args)
    assert R.error_ratio(gs, want_s, bound_s) <= 1.0
    if weighted:
        assert R.error_ratio(gw, want_w, bound_w) <= 1.0


@pytest.mark.parametrize("name,make", SOFTMAX_CASES, ids=[n for n, _ in SOFTMAX_CASES])
def test_softmax_emulation_within_bound(name, make):
    c = make()
    layout = (c["col"], c["row"], c["num_dst"], c["num_src"])
    worst = 0.0
    for seed in range(3):       # three draws of the +-1 ulp v_exp_f32 perturbation
        y = emu_softmax_fwd(c, seed)
        worst = max(worst, R.error_ratio(y, R.softmax_fwd(*layout, c["logits"]),
                                         R.softmax_fwd_bound(*layout, c["logits"])))
        gx = emu_softmax_bwd(c, y)
        worst = max(worst, R.error_ratio(gx, R.softmax_bwd(*layout, y, c["grad_y"]),
                                         R.softmax_bwd_bound(*layout, y, c["grad_y"])))
    assert worst <= 1.0, worst


def test_softmax_reference_masks():
    """Masked logits give exactly 0, fully masked segments NaN -- in the reference and in the
    emulation alike."""
    for kind in ("masked", "all_masked"):
        c = R.softmax_edge_case(kind, False)
        layout = (c["col"], c["row"], c["num_dst"], c["num_src"])
        want = R.softmax_fwd(*layout, c["logits"])
        x = c["logits"].reshape(want.shape)
        dead = np.isneginf(x)
        assert dead.any()
        nan = np.isnan(want)
        if kind == "masked":
            assert not nan.any() and (want[dead] == 0).all()
        else:
            assert nan.any() and (dead | ~nan).all()
        got = emu_softmax_fwd(c)
        assert R.error_ratio(got, want, R.softmax_fwd_bound(*layout, c["logits"])) <= 1.0


@pytest.mark.parametrize("sampler_layout", [True, False])
def test_max_emulation_matches_reference(sampler_layout):
    c = R.tie_case(sampler_layout)
    layout = (c["col"], c["row"], c["num_dst"], c["num_src"])
    assert R.tie_fraction(*layout, c["src"]) >= 0.25
    out, arg = R.max_fwd(*layout, c["src"])
    best, gs = emu_max(c)
    assert np.array_equal(best, out)
    want = R.max_bwd(*layout, arg, c["grad"])
    assert R.error_ratio(gs, want, R.max_bwd_bound(*layout, arg, c["grad"])) <= 1.0
    if sampler_layout:
        assert np.array_equal(gs, want)


def test_max_reference_edges():
    """No in-edges: 0 and no gradient; ties: the lowest edge in segment order, also when the
    edges of a destination are not contiguous."""
    col = np.array([3, 4, 5, 6, 7])
    row = np.array([1, 0, 1, 1, 0])
    src = np.array([[0], [0], [0], [2.], [5.], [2.], [2.], [5.]])
    out, arg = R.max_fwd(col, row, 3, 8, src)
    assert out.tolist() == [[5.], [2.], [0.]] and arg.tolist() == [[1], [0], [-1]]
    g = R.max_bwd(col, row, 3, 8, arg, np.array([[1.], [2.], [3.]]))
    assert g[:, 0].tolist() == [0, 0, 0, 2, 1, 0, 0, 0]
    with pytest.raises(ValueError):
        R.max_fwd(col, row, 1, 8, src)           # row outside [0, num_dst)


# ---- seeded mistakes must break the bounds -------------------------------------------------------
def test_mistake_dropping_last_edge_breaks_bound():
    for name, make in REDUCE_CASES:
        assert _ratio_fwd(make(), False, False, drop_last=True) > 1.0, name


def test_mistake_mean_over_n_plus_one_breaks_bound():
    for name, make in REDUCE_CASES:
        assert _ratio_fwd(make(), True, False, mean_plus_one=True) > 1.0, name
        assert _ratio_fwd(make(), True, True, mean_plus_one=True) > 1.0, name


def test_mistake_weight_head_by_modulo_breaks_bound():
    for name, make in REDUCE_CASES:
        c = make()
        heads = c["w"].reshape(len(c["col"]), -1).shape[1]
        dim = c["src"].reshape(c["num_src"], -1).shape[1]
        if heads == 1 or dim == heads:
            continue                              # c % heads == c / per_head there
        assert _ratio_fwd(c, False, True, head_mod=True) > 1.0, name
        args = (c["col"], c["row"], c["num_dst"], c["num_src"], c["src"], c["w"], False,
                c["grad"])
        gs, _ = emu_reduce_bwd(c, False, True, head_mod=True)
        assert R.error_ratio(gs, R.reduce_bwd(*args)[0], R.reduce_bwd_bound(*args)[0]) > 1.0


@pytest.mark.parametrize("sampler_layout", [True, False])
def test_mistake_tie_to_highest_edge_breaks_bound(sampler_layout):
    c = R.tie_case(sampler_layout)
    layout = (c["col"], c["row"], c["num_dst"], c["num_src"])
    out, arg = R.max_fwd(*layout, c["src"])
    best, gs = emu_max(c, ties_to_highest=True)
    assert np.array_equal(best, out)          # the forward cannot tell
    assert R.error_ratio(gs, R.max_bwd(*layout, arg, c["grad"]),
                         R.max_bwd_bound(*layout, arg, c["grad"])) > 1.0


def test_mistake_softmax_short_sum_breaks_bound():
    for name, make in SOFTMAX_CASES:
        c = make()
        layout = (c["col"], c["row"], c["num_dst"], c["num_src"])
        y = emu_softmax_fwd(c, short_sum=True)
        assert R.error_ratio(y, R.softmax_fwd(*layout, c["logits"]),
                             R.softmax_fwd_bound(*layout, c["logits"])) > 1.0, name
