"""CPU tests of models.DyGFormer: constructor errors, shapes, dropped channels, patch sizes,
forward on CPU tensors against forward_parts on parts built by hand, and the state_dict."""
import pytest
import torch

from gnnflow_amd.models import DyGFormer
from gnnflow_amd.nn import FixedTimeEncode, TimeEncode

L = 8


def _inputs(N=5, dn=6, de=4, length=L, seed=0):
    """Planes shaped like neighbor_cooccurrence(include_self=True)'s, and two tables."""
    g = torch.Generator().manual_seed(seed)
    lengths = torch.randint(1, length + 1, (N, 2), generator=g, dtype=torch.int32)
    filled = torch.arange(length) < lengths.unsqueeze(2)
    nodes = torch.randint(0, 12, (N, 2, length), generator=g).masked_fill(~filled, -1)
    eids = torch.randint(0, 20, (N, 2, length), generator=g).masked_fill(~filled, -1)
    eids[:, :, 0] = -1                                       # the self slot
    delta_t = (torch.rand((N, 2, length), generator=g) * 50).masked_fill(~filled, 0.0)
    delta_t[:, :, 0] = 0.0
    counts = torch.randint(0, length + 1, (N, 2, length, 2), generator=g, dtype=torch.int32)
    counts = counts.masked_fill(~filled.unsqueeze(3), 0)
    node_feats = torch.randn((10, dn), generator=g) if dn else None      # ids 10, 11: no row
    edge_feats = torch.randn((18, de), generator=g) if de else None      # eids 18, 19: no row
    return nodes, eids, delta_t, counts, lengths, node_feats, edge_feats


def _model(dn=6, de=4, **kw):
    torch.manual_seed(1)
    kw.setdefault("max_length", L)
    kw.setdefault("dim_time", 10)
    kw.setdefault("channel_dim", 6)
    kw.setdefault("dim_embed", 12)
    return DyGFormer(dn, de, **kw).eval()


@pytest.mark.parametrize("kw", [dict(dim_node=-1), dict(dim_edge=-1), dict(dim_time=0),
                                dict(channel_dim=0), dict(patch_size=0), dict(num_layers=0),
                                dict(num_heads=0), dict(max_length=1), dict(dim_embed=0),
                                dict(dim_node=2.0), dict(patch_size=True)])
def test_constructor_rejects(kw):
    name = next(iter(kw))
    args = dict(dim_node=4, dim_edge=4)
    args.update(kw)
    with pytest.raises(ValueError, match=name + " must be an int"):
        DyGFormer(**args)


def test_constructor_rejects_a_length_that_is_no_multiple_of_the_patch():
    with pytest.raises(ValueError, match="max_length 32 is not a multiple of patch_size 5"):
        DyGFormer(4, 4, patch_size=5)
    with pytest.raises(ValueError, match="not a multiple of num_heads"):
        DyGFormer(4, 4, channel_dim=5, num_heads=3)
    DyGFormer(0, 4, channel_dim=5, num_heads=3)      # three channels of 5 columns


def test_defaults_and_modules():
    m = DyGFormer(172, 172)
    assert (m.dim_time, m.channel_dim, m.patch_size, m.max_length, m.dim_embed) == \
        (100, 50, 1, 32, 100)
    assert isinstance(m.time_enc, FixedTimeEncode) and not list(m.time_enc.parameters())
    assert m.channels == ["node", "edge", "time", "cooc"] and len(m.blocks) == 2
    assert m.proj["node"].in_features == 172 and m.proj["time"].in_features == 100
    assert m.proj["cooc"].in_features == 50 and m.out_fc.in_features == 200
    assert m.cooc_enc.max_count == 32 and m.blocks[0].w1.out_features == 800
    assert isinstance(DyGFormer(4, 4, learn_time=True).time_enc, TimeEncode)
    p2 = DyGFormer(4, 6, patch_size=2, channel_dim=8, dim_time=10)
    assert [p2.proj[c].in_features for c in p2.channels] == [8, 12, 20, 16]


@pytest.mark.parametrize("patch", [1, 2, L])
def test_shapes_for_every_patch_size(patch):
    m = _model(patch_size=patch)
    x = _inputs()
    score = m(*x)
    assert score.shape == (5, 1) and score.dtype == torch.float32
    assert torch.isfinite(score).all()
    src, dst = m(*x, return_embed=True)
    assert src.shape == dst.shape == (5, 12)
    head = m.edge_predictor
    want = head.out_fc(torch.relu(head.src_fc(src) + head.dst_fc(dst)))
    assert torch.equal(score, want)
    assert m(*_inputs(N=0)).shape == (0, 1)


@pytest.mark.parametrize("dn,de", [(0, 4), (6, 0), (0, 0)])
def test_dropped_channels(dn, de):
    m = _model(dn, de)
    assert ("node" in m.channels) == bool(dn) and ("edge" in m.channels) == bool(de)
    assert m.out_fc.in_features == 6 * len(m.channels)
    x = _inputs(dn=dn, de=de)
    score = m(*x)
    assert score.shape == (5, 1) and torch.isfinite(score).all()
    # a table for a dropped channel is ignored
    junk = torch.full((3, 7), float("nan"))
    y = list(x)
    if not dn:
        y[5] = junk
    if not de:
        y[6] = junk
    assert torch.equal(m(*y), score)


def test_forward_builds_the_parts_forward_parts_takes():
    m = _model()
    nodes, eids, delta_t, counts, lengths, node_feats, edge_feats = _inputs()
    pad = (torch.arange(L) >= lengths.unsqueeze(2)).unsqueeze(3)
    node_x = torch.zeros(5, 2, L, 6)
    edge_x = torch.zeros(5, 2, L, 4)
    for i in range(5):
        for s in range(2):
            for p in range(int(lengths[i, s])):
                if 0 <= nodes[i, s, p] < 10:
                    node_x[i, s, p] = node_feats[nodes[i, s, p]]
                if 0 <= eids[i, s, p] < 18:
                    edge_x[i, s, p] = edge_feats[eids[i, s, p]]
    assert (nodes >= 10).any() and (eids >= 18).any()        # ids without a row are in there
    time_x = m.time_enc(delta_t).masked_fill(pad, 0.0)
    want = m.forward_parts(node_x, edge_x, time_x, counts, lengths)
    assert torch.equal(m(nodes, eids, delta_t, counts, lengths, node_feats, edge_feats), want)
    # what the padded slots hold does not matter to forward: it fills them
    assert torch.equal(m(nodes.masked_fill(pad[..., 0], 3), eids.masked_fill(pad[..., 0], 3),
                         delta_t.masked_fill(pad[..., 0], float("nan")), counts, lengths,
                         node_feats, edge_feats), want)


def test_wrong_shapes():
    m = _model()
    x = _inputs(length=4)
    with pytest.raises(ValueError, match="sequences of 4 slots per side, max_length is 8"):
        m(*x)
    nodes, eids, delta_t, counts, lengths, node_feats, edge_feats = _inputs()
    time_x = torch.zeros(5, 2, L, 10)
    with pytest.raises(ValueError, match="the node part must be"):
        m.forward_parts(torch.zeros(5, 2, L, 5), torch.zeros(5, 2, L, 4), time_x, counts, lengths)
    with pytest.raises(ValueError, match="the time part must be"):
        m.forward_parts(torch.zeros(5, 2, L, 6), torch.zeros(5, 2, L, 4), time_x[:, :, :4],
                        counts, lengths)
    with pytest.raises(ValueError, match="counts must be"):
        m.forward_parts(None, None, time_x, counts[..., 0], lengths)


def test_training_mode_backward_and_learn_time():
    m = _model(learn_time=True, dropout=0.0).train()
    x = _inputs()
    m(*x).sum().backward()
    for name, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert m.time_enc.w.weight.grad.abs().sum() > 0
    fixed = _model(dropout=0.0)
    assert not any(n.startswith("time_enc") for n, _ in fixed.named_parameters())


def test_state_dict_round_trip():
    a, x = _model(patch_size=2), _inputs()
    torch.manual_seed(7)
    b = DyGFormer(6, 4, max_length=L, dim_time=10, channel_dim=6, dim_embed=12,
                  patch_size=2).eval()
    assert not torch.equal(a(*x), b(*x))
    assert "time_enc.weight" in a.state_dict() and "time_enc.bias" in a.state_dict()
    b.load_state_dict(a.state_dict())
    assert torch.equal(a(*x), b(*x))
