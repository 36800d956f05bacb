"""models.DGNN and nn.EdgePredictor on the GPU: the fused predictor against the reference's
recorded run, state-dict names and shapes of the memory configurations, DGNN.forward against a
hand composition of its sub-modules (bit-equal), the memory route over two consecutive batches,
backup / restore / resize, one optimiser step with fused_score on and off, and how often
ops.edge_score is called.  Blocks come from the package's sampler on a tests/synth.py graph of
600 edges: 12 edges per batch (36 roots), fanout 3."""
import numpy as np
import pytest

from tests import edge_score_ref as ES
from tests import synth
from tests.test_models_cpu import dgnn_fixture, dgnn_kwargs, load_predictor, predictor_fixture

pytestmark = pytest.mark.gpu

N, E, BATCH, T_MAX = 200, 600, 12, 1000.0
CONFIGS = ["tgat", "tgn_nonode", "tgn_node32", "dysat"]


class _World:
    """The graph, one sampler per snapshot count, and seeded feature tables."""

    def __init__(self):
        import torch
        from gnnflow_amd import DynamicGraph
        self.src, self.dst, self.ts, eid = synth.powerlaw_graph(N, E, seed=5, t_max=T_MAX)
        self.graph = DynamicGraph(1 << 20, 64 << 20, "cuda", 16, 64, "insert")
        synth.ingest_chunks(self.graph, self.src, self.dst, self.ts, eid, 200, add_reverse=True)
        rng = np.random.RandomState(6)
        self.nfeat = torch.from_numpy(rng.randn(N, 32).astype(np.float32)).cuda()
        self.efeat = torch.from_numpy(rng.randn(E, 16).astype(np.float32)).cuda()
        self.neg = rng.randint(0, N, size=E).astype(np.int64)
        self.samplers = {}

    def mfgs(self, kw, batch):
        """Blocks of batch number `batch` (counted from edge 400 on) with their features."""
        from gnnflow_amd import TemporalSampler
        key = (kw["num_layers"], kw["num_snapshots"])
        if key not in self.samplers:
            self.samplers[key] = TemporalSampler(self.graph, [3] * key[0], "recent", key[1],
                                                 300.0 if key[1] > 1 else 0.0)
        lo = 400 + batch * BATCH
        sl = slice(lo, lo + BATCH)
        roots = np.concatenate([self.src[sl], self.dst[sl], self.neg[sl]])
        mfgs = self.samplers[key].sample(roots, np.tile(self.ts[sl], 3))
        assert len(mfgs) == key[0] and all(len(m) == key[1] for m in mfgs)
        assert mfgs[-1][0].num_dst_nodes() == 3 * BATCH and mfgs[0][0].num_edges() > 0
        for l, layer in enumerate(mfgs):
            for b in layer:
                b.edata['f'] = self.efeat[b.edata['ID']]
                if l == 0 and kw["dim_node"]:
                    b.srcdata['h'] = self.nfeat[b.srcdata['ID']]
        return mfgs


@pytest.fixture(scope="module")
def world():
    return _World()


def _model(name, seed=11, **over):
    import torch
    from gnnflow_amd.models import DGNN
    kw = dict(dgnn_kwargs(dgnn_fixture(), name), **over)
    torch.manual_seed(seed)
    return DGNN(**kw).cuda(), kw


def _prepare(model, mfgs):
    """What the training loop does ahead of forward() with memory."""
    if model.has_memory():
        b = mfgs[0][0]
        model.memory.prepare_input(b)
        model.last_updated = model.memory_updater(b)


def _np(t):
    return t.detach().cpu().numpy()


# ---- the predictor against the reference's recorded run -------------------------------------
def test_fused_edge_predictor_reproduces_the_recorded_reference_run():
    """Twice the edge_score bounds propagated through the two Linears (PredictorReference: the
    float64 module from the recorded weights): the recorded fp32 run and the fused run are each
    within the bounds of the float64 module, so at most twice the bounds apart."""
    import torch
    fix = predictor_fixture()
    state = {k[len("state."):]: v for k, v in fix.items() if k.startswith("state.")}
    ref = ES.PredictorReference(state, fix["h"], np.r_[np.ones(7), -2 * np.ones(7)])
    assert ref.mask_is_stable
    model = load_predictor(fix).cuda()
    model.fused_score = True
    h = torch.from_numpy(fix["h"]).cuda().requires_grad_(True)
    pos, neg = model(h)
    assert pos.shape == neg.shape == (7, 1)
    (pos.sum() - 2 * neg.sum()).backward()
    grads = {k: _np(v.grad) for k, v in model.named_parameters()}
    grads["h"] = _np(h.grad)
    ratios = {"pos": ES.error_ratio(_np(pos), fix["pos"], 2 * ref.b_pos),
              "neg": ES.error_ratio(_np(neg), fix["neg"], 2 * ref.b_neg)}
    for k, v in grads.items():
        ratios[k] = ES.error_ratio(v, fix["grad." + k], 2 * ref.bounds[k])
    own = ref.ratios(_np(pos), _np(neg), grads)
    print("\n[difference / (2 x bound)] fused - recorded: {:.3g}; [error/bound] fused - float64: "
          "{:.3g}".format(max(ratios.values()), max(own.values())))
    assert max(ratios.values()) <= 1.0, ratios


def test_edge_predictor_rejects_rows_not_a_multiple_of_three_on_the_gpu():
    import torch
    from gnnflow_amd import nn as gnn
    model = gnn.EdgePredictor(8).cuda()
    model.fused_score = True
    with pytest.raises(ValueError, match="multiple of 3"):
        model(torch.zeros(10, 8, device="cuda"))
    pos, neg = model(torch.zeros(0, 8, device="cuda"))
    assert pos.shape == neg.shape == (0, 1)


@pytest.mark.parametrize("fused", [False, True])
def test_edge_score_calls_per_forward(fused, world, monkeypatch):
    """Fused: exactly one ops.edge_score call per forward.  Not fused, or CPU tensors: none."""
    import torch
    from gnnflow_amd import nn as gnn
    from gnnflow_amd import ops
    calls = []
    real = ops.edge_score
    monkeypatch.setattr(ops, "edge_score", lambda *a, **k: calls.append(1) or real(*a, **k))
    model, kw = _model("tgat")
    model.eval()
    model.edge_predictor.fused_score = fused
    for batch in range(2):
        pos, neg = model(world.mfgs(kw, batch))
        assert pos.shape == neg.shape == (BATCH, 1)
        assert len(calls) == ((batch + 1) if fused else 0)
    assert model(world.mfgs(kw, 0), return_embed=True).shape == (3 * BATCH, kw["dim_embed"])
    n = len(calls)
    cpu = gnn.EdgePredictor(8)
    cpu.fused_score = fused
    cpu(torch.zeros(6, 8))
    assert len(calls) == n


# ---- state dict of the memory configurations ------------------------------------------------
@pytest.mark.parametrize("name", ["tgn_nonode", "tgn_node32"])
def test_dgnn_state_dict_with_memory_matches_the_reference_fixture(name):
    import torch
    from gnnflow_amd import nn as gnn
    from gnnflow_amd.memory import Memory
    fix = dgnn_fixture()
    model, kw = _model(name)
    got = {k: list(v.shape) for k, v in model.state_dict().items()}
    assert got == fix["configs"][name]
    assert model.has_memory() and model.last_updated is None
    assert isinstance(model.memory, Memory) and isinstance(model.memory_updater,
                                                           gnn.GRUMemoryUpdater)
    cur = torch.device("cuda", torch.cuda.current_device())
    assert model.memory.device == cur and model.memory.node_memory.device == cur
    assert tuple(model.memory.node_memory.shape) == (kw["num_nodes"], kw["dim_memory"])
    with pytest.raises(NotImplementedError):
        _model(name, kvstore_client=object())


# ---- forward ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONFIGS)
def test_forward_is_bit_equal_to_the_hand_composition(name, world):
    """dgnn.py:126-143 spelled out with the model's own sub-modules."""
    import torch
    model, kw = _model(name)
    model.eval()
    L, S = kw["num_layers"], kw["num_snapshots"]
    with torch.no_grad():
        mfgs = world.mfgs(kw, 0)
        _prepare(model, mfgs)
        pos, neg = model(mfgs)
        embed = model(mfgs, return_embed=True)

        hand = world.mfgs(kw, 0)
        _prepare(model, hand)
        last = []
        for l in range(L):
            for h in range(S):
                rst = model.layers["l{}h{}".format(l, h)](hand[l][h])
                if l != L - 1:
                    hand[l + 1][h].srcdata['h'] = rst
                else:
                    last.append(rst)
        want = last[0] if S == 1 else model.combiner(torch.stack(last, dim=0))[0][-1, :, :]
        want_pos, want_neg = model.edge_predictor(want)
    assert tuple(embed.shape) == (3 * BATCH, kw["dim_embed"]) and embed.abs().sum() > 0
    assert torch.equal(embed, want)
    assert torch.equal(pos, want_pos) and torch.equal(neg, want_neg)
    assert tuple(pos.shape) == tuple(neg.shape) == (BATCH, 1)


# ---- memory ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tgn_nonode", "tgn_node32"])
def test_memory_route_over_two_batches(name, world):
    """prepare_input -> memory_updater -> layers -> update_mem_mail(**last_updated, ...) twice.
    With one negative per edge the roots are [src | dst | neg] and update_mem_mail writes the
    source and destination two thirds of last_updated_nid (memory.py:192-269): exactly those
    rows of node_memory change, each to the memory of its last occurrence; then backup /
    restore round-trip and resize grows the tables."""
    import torch
    model, kw = _model(name)
    model.eval()
    mem = model.memory
    assert not mem.node_memory.any()
    for batch in range(2):
        mfgs = world.mfgs(kw, batch)
        with torch.no_grad():
            _prepare(model, mfgs)
            last = model.last_updated
            assert torch.equal(last["last_updated_nid"], mfgs[0][0].srcdata['ID'][:mfgs[0][0].num_dst_nodes()])
            before = mem.node_memory.clone()
            pos, neg = model(mfgs)
            assert torch.equal(mem.node_memory, before)        # forward() itself writes nothing
            mem.update_mem_mail(**last, edge_feats=None, neg_sample_ratio=1)
        nid = _np(last["last_updated_nid"])
        assert len(nid) == 3 * BATCH
        named = nid[:2 * BATCH]
        after, was = _np(mem.node_memory), _np(before)
        rest = np.setdiff1d(np.arange(kw["num_nodes"]), named)
        assert np.array_equal(after[rest], was[rest])
        new = _np(last["last_updated_memory"])
        for v in np.unique(named):
            p = np.flatnonzero(named == v)[-1]
            assert np.array_equal(after[v], new[p]) and not np.array_equal(after[v], was[v])
        assert torch.isfinite(pos).all() and torch.isfinite(neg).all()
    # the second batch read what the first wrote
    assert mfgs[0][0].srcdata['mem'].abs().sum() > 0
    backup = model.backup_memory()
    assert set(backup) == {"node_memory", "node_memory_ts", "mailbox", "mailbox_ts"}
    saved = {k: v.clone() for k, v in backup.items()}
    model.reset()
    assert not mem.node_memory.any() and not mem.mailbox.any()
    assert all(torch.equal(backup[k], saved[k]) for k in saved)      # a copy, not a view
    model.restore_memory(backup)
    for k, v in saved.items():
        assert torch.equal(getattr(mem, k), v)
    model.resize(kw["num_nodes"] + 50)
    assert mem.num_nodes == kw["num_nodes"] + 50
    assert tuple(mem.node_memory.shape) == (kw["num_nodes"] + 50, kw["dim_memory"])
    assert tuple(mem.mailbox.shape)[0] == tuple(mem.mailbox_ts.shape)[0] == kw["num_nodes"] + 50
    assert torch.equal(mem.node_memory[:kw["num_nodes"]], saved["node_memory"])
    assert not mem.node_memory[kw["num_nodes"]:].any()
    model.resize(10)                                                  # never shrinks
    assert mem.num_nodes == kw["num_nodes"] + 50


@pytest.mark.parametrize("name", ["tgat", "dysat"])
def test_memory_calls_are_no_ops_without_memory(name):
    model, _ = _model(name)
    assert not model.has_memory()
    assert model.reset() is None and model.resize(10 ** 6) is None
    assert model.backup_memory() == {} and model.restore_memory({}) is None


# ---- one optimiser step ------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONFIGS)
def test_one_optimiser_step_fused_and_not(name, world):
    """Every parameter gets a finite gradient and the step moves the model, fused_score on and off; the
    two losses agree within the propagated bound: the logits of either path are within b_pos /
    b_neg (PredictorReference, from the embedding both paths share) of the float64 head, BCE
    with logits is a mean of B terms of slope at most 1 in its logit, and evaluating it in fp32
    costs each side at most gamma_{B+8} of its value (B - 1 adds, at most 8 roundings inside a
    term max(x, 0) - x y + log1p(exp(-|x|)), all terms non-negative)."""
    import torch
    import torch.nn.functional as F
    losses = {}
    for fused in (False, True):
        model, kw = _model(name, dropout=0.0, att_dropout=0.0)
        model.train()
        model.edge_predictor.fused_score = fused
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        mfgs = world.mfgs(kw, 1)
        with torch.no_grad():
            _prepare(model, mfgs)
            embed = model(mfgs, return_embed=True)
        mfgs = world.mfgs(kw, 1)
        _prepare(model, mfgs)
        opt.zero_grad()
        pos, neg = model(mfgs)
        loss = F.binary_cross_entropy_with_logits(pos, torch.ones_like(pos)) + \
            F.binary_cross_entropy_with_logits(neg, torch.zeros_like(neg))
        loss.backward()
        before = {k: v.detach().clone() for k, v in model.named_parameters()}
        for k, v in model.named_parameters():
            assert v.grad is not None, k
            assert torch.isfinite(v.grad).all(), k
        opt.step()
        moved = [k for k, v in model.named_parameters() if not torch.equal(v, before[k])]
        assert moved and all(torch.isfinite(v).all() for v in model.parameters())
        losses[fused] = (float(loss.detach()), _np(embed), {k: _np(v) for k, v in before.items()
                                                    if k.startswith("edge_predictor.")})
    (lu, eu, su), (lf, ef, sf) = losses[False], losses[True]
    assert np.array_equal(eu, ef) and all(np.array_equal(su[k], sf[k]) for k in su)
    state = {k[len("edge_predictor."):]: v for k, v in su.items()}
    ref = ES.PredictorReference(state, eu, np.zeros(2 * BATCH))
    bound = 2 * (ref.b_pos.mean() + ref.b_neg.mean()) + 2 * ES.gamma(BATCH + 8) * max(lu, lf)
    print("\n[loss] {}: unfused {:.9g}, fused {:.9g}, difference / bound = {:.3g}".format(
        name, lu, lf, abs(lu - lf) / bound))
    assert abs(lu - lf) <= bound
