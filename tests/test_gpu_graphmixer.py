"""GPU: nn.FixedTimeEncode and models.GraphMixer at n = 12 rows, K = 4 tokens and every width 8:
the frozen time encoding is ops.time_encode on its buffers bit for bit, the model's shapes, its
indifference to what the padded slots hold, and finite non-zero gradients on every parameter."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

N, K, D = 12, 4, 8


def _inputs(seed=0, dim_node=D):
    g = torch.Generator().manual_seed(seed)
    edge_x = torch.randn(N, K, D, generator=g).cuda()
    delta_t = (torch.rand(N, K, generator=g) * 1000).cuda()
    lengths = torch.tensor([0, 1, 2, 3, 4, 4, 2, 1, 3, 4, 0, 2], dtype=torch.int32).cuda()
    node_x = torch.randn(N, dim_node, generator=g).cuda() if dim_node else None
    nbr_mean = torch.randn(N, dim_node, generator=g).cuda() if dim_node else None
    return edge_x, delta_t, lengths, node_x, nbr_mean


def _model(dim_node=D, **kw):
    from gnnflow_amd.models import GraphMixer
    torch.manual_seed(1)
    return GraphMixer(dim_node, D, dim_time=D, dim_embed=D, num_tokens=K, **kw).cuda()


def test_fixed_time_encode_is_time_encode_on_its_buffers():
    from gnnflow_amd import FixedTimeEncode, ops
    for dim in (1, 8, 100):
        enc = FixedTimeEncode(dim).cuda()
        assert list(enc.parameters()) == []
        assert sorted(dict(enc.named_buffers())) == ["bias", "weight"]
        assert sorted(enc.state_dict()) == ["bias", "weight"]
        want_w = 1 / 10 ** np.linspace(0, 9, dim, dtype=np.float32)
        assert np.array_equal(enc.weight.cpu().numpy().reshape(-1), want_w)
        assert enc.weight[0, 0] == 1.0 and not enc.bias.any()
        if dim > 1:
            assert abs(float(enc.weight[-1, 0]) / 1e-9 - 1) < 1e-5
        dt = (torch.rand(N, K) * 1e4).cuda()
        out = enc(dt)
        assert tuple(out.shape) == (N, K, dim) and out.dtype == torch.float32
        want = ops.time_encode(dt.reshape(-1), enc.weight, enc.bias).reshape(N, K, dim)
        assert torch.equal(out.view(torch.int32), want.view(torch.int32))
        assert torch.allclose(out, torch.cos(dt[..., None] * enc.weight.reshape(-1)), atol=1e-3)
        assert not out.requires_grad


def test_forward_shapes():
    model = _model().eval()
    args = _inputs()
    embed = model(*args, return_embed=True)
    assert tuple(embed.shape) == (N, D) and embed.dtype == torch.float32
    pos, neg = model(*args)
    assert tuple(pos.shape) == (N // 3, 1) and tuple(neg.shape) == (N // 3, 1)
    assert torch.isfinite(embed).all() and torch.isfinite(pos).all() and torch.isfinite(neg).all()
    assert len(model.mixers) == 2 and list(model.time_enc.parameters()) == []
    with pytest.raises(ValueError, match="num_tokens"):
        model(args[0][:, :3], args[1][:, :3], *args[2:])


def test_padded_slots_do_not_reach_the_output():
    model = _model().eval()
    edge_x, delta_t, lengths, node_x, nbr_mean = _inputs()
    a = model(edge_x, delta_t, lengths, node_x, nbr_mean, return_embed=True)
    padding = torch.arange(K, device="cuda") >= lengths[:, None]
    assert padding.any() and (~padding).any()
    for junk in (1e30, float("nan"), float("-inf")):
        e2 = edge_x.masked_fill(padding[:, :, None], junk)
        t2 = delta_t.masked_fill(padding, junk)
        b = model(e2, t2, lengths, node_x, nbr_mean, return_embed=True)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # and a filled slot does
    e3 = edge_x.clone()
    e3[4, 0] += 1.0
    c = model(e3, delta_t, lengths, node_x, nbr_mean, return_embed=True)
    assert not torch.equal(a[4], c[4])


def test_gradients_reach_every_parameter():
    model = _model().train()
    pos, neg = model(*_inputs())
    loss = torch.nn.functional.binary_cross_entropy_with_logits(pos, torch.ones_like(pos)) + \
        torch.nn.functional.binary_cross_entropy_with_logits(neg, torch.zeros_like(neg))
    loss.backward()
    names = [n for n, _ in model.named_parameters()]
    assert any(n.startswith("mixers.1.token_mlp") for n in names) and "link_in.weight" in names
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        assert torch.isfinite(p.grad).all() and p.grad.abs().sum() > 0, name


def test_without_node_features():
    model = _model(dim_node=0).eval()
    edge_x, delta_t, lengths, _, _ = _inputs(dim_node=0)
    assert model.out_fc.in_features == D
    embed = model(edge_x, delta_t, lengths, return_embed=True)
    assert tuple(embed.shape) == (N, D) and torch.isfinite(embed).all()
    pos, neg = model(edge_x, delta_t, lengths, None, None)
    assert tuple(pos.shape) == (N // 3, 1) and tuple(neg.shape) == (N // 3, 1)
