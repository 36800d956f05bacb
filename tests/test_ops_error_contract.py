"""The error contract of gnnflow_amd.ops, frozen: for every public op, every exception its Python
body can raise without a GPU -- type and full message -- and, where several arguments are wrong
at once, which one fires first.  One table; CPU (and meta) tensors only, no native library."""
import pytest
import torch

from gnnflow_amd import ops

F32, F64, BF16, I64, I32 = (torch.float32, torch.float64, torch.bfloat16, torch.int64,
                            torch.int32)


def Z(*shape, dtype=F32, device="cpu"):
    return torch.zeros(*shape, dtype=dtype, device=device)


def M(*shape, dtype=F32):
    """A tensor on another device class (and of any size) without a GPU."""
    return torch.empty(*shape, dtype=dtype, device="meta")


class _Block:
    """What the block ops read before they launch anything."""

    def __init__(self, num_src, num_dst, num_edges, segments=None):
        self.n, self.seg = (num_src, num_dst, num_edges), segments

    def num_src_nodes(self):
        return self.n[0]

    def num_dst_nodes(self):
        return self.n[1]

    def num_edges(self):
        return self.n[2]

    def segments(self):
        if self.seg is None:
            raise AssertionError("the op looked at the block's edges before validating")
        return self.seg


B = _Block(12, 5, 20)
# the sampler's layout with every edge into destination 0: reaches the Functions' own checks
BSEG = _Block(12, 5, 20, (torch.tensor([0, 20, 20, 20, 20, 20]), None, None))

Q, K, V = Z(5, 2, 3), Z(20, 2, 3), Z(20, 2, 3)               # block_attention
FEAT, EL, ER = Z(12, 2, 3), Z(12, 2), Z(5, 2)                # block_gat
T, TW, TB = Z(4), Z(3, 1), Z(3)                              # time_encode_cat
SRC, DST, CAND, W, BIAS = Z(4, 3), Z(8, 3), Z(10, 3), Z(3), Z(1)      # edge_score, edge_rank
X, G, BE = Z(4, 6), Z(6), Z(6)                               # dropout_relu_layer_norm
GI, GH, HX = Z(4, 9), Z(4, 9), Z(4, 3)                       # gru_cell
POS, NEG = Z(4), Z(8)                                        # link_metrics, link_loss
NODES = Z(2, 3, 5, dtype=I64)                                # walk_position_counts

ALMOST_ONE = 1 - 2.0 ** -30      # < 1 in float64, 1 in float32

att, gat, drln = ops.block_attention, ops.block_gat, ops.dropout_relu_layer_norm
tec, te, es, er = ops.time_encode_cat, ops.time_encode, ops.edge_score, ops.edge_rank
gru, lm, ll = ops.gru_cell, ops.link_metrics, ops.link_loss
wpc, wargs = ops.walk_position_counts, ops.check_walk_position_counts_args

P_RANGE = "dropout_p must be in [0, 1), got {}"
P_ROUNDS = "dropout_p rounds to 1 in float32"
SEED_RANGE = "dropout_seed must be in [0, 2**64), got 18446744073709551616"
SEED_NEEDED = "dropout_p > 0 needs a dropout_seed"
GAT_DTYPES = ("block_gat computes in float32 and takes feat float32 or bfloat16 with el and er "
              "float32, feat is {}, el is {} and er is {}")

CASES = [
    # ---- edge_softmax, block_reduce, block_max
    ("edge_softmax-rows", lambda: ops.edge_softmax(B, Z(19)),
     ValueError, "logits must have one row per edge"),
    ("edge_softmax-rows-before-dtype", lambda: ops.edge_softmax(BSEG, Z(19, dtype=F64)),
     ValueError, "logits must have one row per edge"),
    ("edge_softmax-dtype", lambda: ops.edge_softmax(BSEG, Z(20, dtype=F64)),
     TypeError, "block ops compute in float32, got torch.float64"),
    ("block_reduce-src-type", lambda: ops.block_reduce(B, [1.0]),
     TypeError, "src must be a tensor, got list"),
    ("block_reduce-src-dtype", lambda: ops.block_reduce(B, Z(12, 6, dtype=F64)),
     TypeError, "block_reduce computes in float32 and takes src float32 or bfloat16, src is "
                "torch.float64"),
    ("block_reduce-weight-type", lambda: ops.block_reduce(B, Z(12, 6), 1.0),
     TypeError, "edge_weight must be a tensor or None, got float"),
    ("block_reduce-weight-dtype", lambda: ops.block_reduce(B, Z(12, 6, dtype=BF16), Z(20, 2, dtype=BF16)),
     TypeError, "block_reduce computes in float32 and takes edge_weight float32 (src float32 or "
                "bfloat16), src is torch.bfloat16 and edge_weight is torch.bfloat16"),
    ("block_reduce-rows", lambda: ops.block_reduce(B, Z(11, 6)),
     ValueError, "src must have one row per source node"),
    ("block_reduce-heads", lambda: ops.block_reduce(BSEG, Z(12, 6), Z(20, 4)),
     ValueError, "feature size 6 is not a multiple of the 4 edge-weight heads"),
    ("block_reduce-src-dtype-before-weight-type",
     lambda: ops.block_reduce(B, Z(12, 6, dtype=F64), 1.0),
     TypeError, "block_reduce computes in float32 and takes src float32 or bfloat16, src is "
                "torch.float64"),
    ("block_reduce-weight-dtype-before-rows",
     lambda: ops.block_reduce(B, Z(11, 6), Z(20, 2, dtype=F64)),
     TypeError, "block_reduce computes in float32 and takes edge_weight float32 (src float32 or "
                "bfloat16), src is torch.float32 and edge_weight is torch.float64"),
    ("block_max-src-type", lambda: ops.block_max(B, None),
     TypeError, "src must be a tensor, got NoneType"),
    ("block_max-src-dtype", lambda: ops.block_max(B, Z(12, 6, dtype=torch.float16)),
     TypeError, "block_max computes in float32 and takes src float32 or bfloat16, src is "
                "torch.float16"),
    ("block_max-rows", lambda: ops.block_max(B, Z(13, 6)),
     ValueError, "src must have one row per source node"),
    ("block_max-dtype-before-rows", lambda: ops.block_max(B, Z(13, 6, dtype=F64)),
     TypeError, "block_max computes in float32 and takes src float32 or bfloat16, src is "
                "torch.float64"),
    ("block_max-int-dtype-before-rows", lambda: ops.block_max(B, Z(0, 6, dtype=I64)),
     TypeError, "block_max computes in float32 and takes src float32 or bfloat16, src is "
                "torch.int64"),
    ("grad_as", lambda: ops._grad_as(Z(3), BF16),
     TypeError, "the gradient of a torch.bfloat16 output is torch.float32"),

    # ---- block_attention
    ("att-p-negative", lambda: att(B, Q, K, V, dropout_p=-0.1, dropout_seed=1),
     ValueError, P_RANGE.format("-0.1")),
    ("att-p-nan", lambda: att(B, Q, K, V, dropout_p=float("nan"), dropout_seed=1),
     ValueError, P_RANGE.format("nan")),
    ("att-p-one", lambda: att(B, Q, K, V, dropout_p=1.0, dropout_seed=1),
     ValueError, P_RANGE.format("1.0")),
    ("att-p-rounds", lambda: att(B, Q, K, V, dropout_p=ALMOST_ONE, dropout_seed=1),
     ValueError, P_ROUNDS),
    ("att-seed-range", lambda: att(B, Q, K, V, dropout_p=0.5, dropout_seed=2 ** 64),
     ValueError, SEED_RANGE),
    ("att-seed-range-without-dropout", lambda: att(B, Q, K, V, dropout_seed=2 ** 64),
     ValueError, SEED_RANGE),
    ("att-seed-negative", lambda: att(B, Q, K, V, dropout_p=0.5, dropout_seed=-1),
     ValueError, "dropout_seed must be in [0, 2**64), got -1"),
    ("att-seed-needed", lambda: att(B, Q, K, V, dropout_p=0.5),
     ValueError, SEED_NEEDED),
    ("att-rounds-before-seed-needed", lambda: att(B, Q, K, V, dropout_p=ALMOST_ONE),
     ValueError, P_ROUNDS),
    ("att-dtypes", lambda: att(B, Q, K.double(), V),
     TypeError, "block_attention takes q, k and v all float32 or all bfloat16 (block ops compute "
                "in float32), got torch.float32, torch.float64 and torch.float32"),
    ("att-q-rows", lambda: att(B, Q[:4], K, V),
     ValueError, "q must have one row per destination node"),
    ("att-kv-rows", lambda: att(B, Q, K, V[:19]),
     ValueError, "k and v must have one row per edge"),
    ("att-heads-columns", lambda: att(B, Z(5, 6), Z(20, 6), Z(20, 6), heads=4),
     ValueError, "q has 6 columns, not a multiple of heads=4"),
    ("att-rank", lambda: att(B, Q, Z(20, 6), V),
     ValueError, "k must be [rows, H, D] (or [rows, H * D] with heads=), got (20, 6)"),
    ("att-differ", lambda: att(B, Q, Z(20, 2, 4), V),
     ValueError, "q, k and v differ in [H, D]: (2, 3), (2, 4), (2, 3)"),
    ("att-heads-mismatch", lambda: att(B, Q, K, V, heads=3),
     ValueError, "heads=3 but the inputs have 2 heads"),
    ("att-empty-width", lambda: att(B, Z(5, 0, 3), Z(20, 0, 3), Z(20, 0, 3)),
     ValueError, "block_attention needs H >= 1 and D >= 1"),
    ("att-width", lambda: att(B, Z(5, 2, 513), Z(20, 2, 513), Z(20, 2, 513)),
     ValueError, "H * D = 1026 exceeds the limit of 1024"),
    ("att-p-before-dtypes", lambda: att(B, Q, K.double(), V, dropout_p=2.0, dropout_seed=1),
     ValueError, P_RANGE.format("2.0")),
    ("att-seed-needed-before-dtypes", lambda: att(B, Q.to(BF16), K, V, dropout_p=0.5),
     ValueError, SEED_NEEDED),
    ("att-dtypes-before-rows", lambda: att(B, Q[:4].to(BF16), K, V),
     TypeError, "block_attention takes q, k and v all float32 or all bfloat16 (block ops compute "
                "in float32), got torch.bfloat16, torch.float32 and torch.float32"),
    ("att-q-rows-before-kv-rows", lambda: att(B, Q[:4], K[:3], V),
     ValueError, "q must have one row per destination node"),
    ("att-rows-before-rank", lambda: att(B, Q, Z(19, 6), V),
     ValueError, "k and v must have one row per edge"),

    # ---- block_gat
    ("gat-p-negative", lambda: gat(B, FEAT, EL, ER, dropout_p=-1, dropout_seed=1),
     ValueError, P_RANGE.format("-1.0")),
    ("gat-p-nan", lambda: gat(B, FEAT, EL, ER, dropout_p=float("nan"), dropout_seed=1),
     ValueError, P_RANGE.format("nan")),
    ("gat-p-one", lambda: gat(B, FEAT, EL, ER, dropout_p=1.0, dropout_seed=1),
     ValueError, P_RANGE.format("1.0")),
    ("gat-p-rounds", lambda: gat(B, FEAT, EL, ER, dropout_p=ALMOST_ONE, dropout_seed=1),
     ValueError, P_ROUNDS),
    ("gat-seed-range", lambda: gat(B, FEAT, EL, ER, dropout_p=0.5, dropout_seed=2 ** 64),
     ValueError, SEED_RANGE),
    ("gat-seed-range-without-dropout", lambda: gat(B, FEAT, EL, ER, dropout_seed=2 ** 64),
     ValueError, SEED_RANGE),
    ("gat-seed-needed", lambda: gat(B, FEAT, EL, ER, dropout_p=0.25),
     ValueError, SEED_NEEDED),
    ("gat-type", lambda: gat(B, FEAT, EL.numpy(), ER),
     TypeError, "el must be a tensor, got ndarray"),
    ("gat-dtypes", lambda: gat(B, FEAT.double(), EL, ER),
     TypeError, GAT_DTYPES.format("torch.float64", "torch.float32", "torch.float32")),
    ("gat-el-dtype", lambda: gat(B, FEAT.to(BF16), EL.to(BF16), ER),
     TypeError, GAT_DTYPES.format("torch.bfloat16", "torch.bfloat16", "torch.float32")),
    ("gat-feat-rank", lambda: gat(B, Z(12, 6), EL, ER),
     ValueError, "feat must be [num_src, H, D], got (12, 6)"),
    ("gat-el-rank", lambda: gat(B, FEAT, Z(12, 2, 1), ER),
     ValueError, "el and er must be [rows, H], got (12, 2, 1) and (5, 2)"),
    ("gat-src-rows", lambda: gat(B, FEAT, EL[:11], ER),
     ValueError, "feat and el must have one row per source node"),
    ("gat-dst-rows", lambda: gat(B, FEAT, EL, ER[:4]),
     ValueError, "er must have one row per destination node"),
    ("gat-heads", lambda: gat(B, FEAT, Z(12, 3), ER),
     ValueError, "feat, el and er differ in H: 2, 3, 2"),
    ("gat-empty-width", lambda: gat(B, Z(12, 2, 0), EL, ER),
     ValueError, "block_gat needs H >= 1 and D >= 1"),
    ("gat-width", lambda: gat(B, Z(12, 2, 513), EL, ER),
     ValueError, "H * D = 1026 exceeds the limit of 1024"),
    ("gat-device", lambda: gat(B, FEAT, M(12, 2), ER),
     ValueError, "feat is on cpu, el on meta, er on cpu"),
    ("gat-gpu", lambda: gat(B, FEAT, EL, ER),
     ValueError, "block_gat runs on the GPU, the inputs are on cpu"),
    ("gat-gpu-meta", lambda: gat(B, M(12, 2, 3), M(12, 2), M(5, 2)),
     ValueError, "block_gat runs on the GPU, the inputs are on meta"),
    ("gat-p-before-type", lambda: gat(B, FEAT.numpy(), EL, ER, dropout_p=1.5),
     ValueError, P_RANGE.format("1.5")),
    ("gat-seed-needed-before-type", lambda: gat(B, None, EL, ER, dropout_p=0.5),
     ValueError, SEED_NEEDED),
    ("gat-type-before-dtypes", lambda: gat(B, FEAT.double(), EL, 3),
     TypeError, "er must be a tensor, got int"),
    ("gat-dtypes-before-rank", lambda: gat(B, Z(12, 6), EL.half(), ER),
     TypeError, GAT_DTYPES.format("torch.float32", "torch.float16", "torch.float32")),
    ("gat-width-before-device", lambda: gat(B, Z(12, 2, 513), M(12, 2), ER),
     ValueError, "H * D = 1026 exceeds the limit of 1024"),
    ("gat-device-before-gpu", lambda: gat(B, FEAT, EL, M(5, 2)),
     ValueError, "feat is on cpu, el on cpu, er on meta"),

    # ---- time_encode_cat, time_encode
    ("tec-out-dtype", lambda: tec((), T, TW, TB, out_dtype=torch.float16),
     ValueError, "out_dtype must be None, torch.float32 or torch.bfloat16, got torch.float16"),
    ("tec-parts", lambda: tec((Z(4, 2),) * 3, T, TW, TB),
     ValueError, "time_encode_cat takes at most two parts, got 3"),
    ("tec-type", lambda: tec((), T, 1.0, TB),
     TypeError, "weight must be a tensor, got float"),
    ("tec-part-type", lambda: tec((Z(4, 2), Z(4, 2).numpy()), T, TW, TB),
     TypeError, "parts[1] must be a tensor, got ndarray"),
    ("tec-dtype", lambda: tec((), T, TW, TB.double()),
     TypeError, "time_encode_cat computes in float32, bias is torch.float64"),
    ("tec-part-dtype", lambda: tec((Z(4, 2, dtype=BF16),), T, TW, TB),
     TypeError, "time_encode_cat computes in float32, parts[0] is torch.bfloat16"),
    ("tec-t-rank", lambda: tec((), Z(4, 2), TW, TB),
     ValueError, "t must be [n] or [n, 1], got (4, 2)"),
    ("tec-bias-rank", lambda: tec((), T, TW, Z(3, 1)),
     ValueError, "bias must be [T], got (3, 1)"),
    ("tec-empty", lambda: tec((), T, Z(0, 1), Z(0)),
     ValueError, "time_encode_cat needs T >= 1"),
    ("tec-weight-shape", lambda: tec((), T, Z(4, 1), TB),
     ValueError, "weight must be [T, 1] or [T] with T = 3, got (4, 1)"),
    ("tec-part-rank", lambda: tec((Z(4),), T, TW, TB),
     ValueError, "parts[0] must be [n, W], got (4,)"),
    ("tec-part-rows", lambda: tec((Z(4, 2), Z(5, 2)), Z(4, 1), TW, TB),
     ValueError, "parts[1] has 5 rows, t has 4"),
    ("tec-device", lambda: tec((), T, TW, M(3)),
     ValueError, "bias is on meta, t on cpu"),
    ("tec-part-device", lambda: tec((M(4, 2),), T, TW, TB),
     ValueError, "parts[0] is on meta, t on cpu"),
    ("tec-gpu", lambda: tec((Z(4, 2),), T, TW, TB),
     ValueError, "time_encode_cat runs on the GPU, the inputs are on cpu"),
    ("te-gpu", lambda: te(T, Z(3), TB, out_dtype=BF16),
     ValueError, "time_encode_cat runs on the GPU, the inputs are on cpu"),
    ("te-type", lambda: te([0.0], TW, TB),
     TypeError, "t must be a tensor, got list"),
    ("te-out-dtype-before-type", lambda: te(None, TW, TB, out_dtype=F64),
     ValueError, "out_dtype must be None, torch.float32 or torch.bfloat16, got torch.float64"),
    ("te-weight-shape-before-device", lambda: te(T, Z(3, 2), M(3)),
     ValueError, "weight must be [T, 1] or [T] with T = 3, got (3, 2)"),
    ("tec-out-dtype-before-parts", lambda: tec((Z(4, 2),) * 3, T, TW, TB, out_dtype=I64),
     ValueError, "out_dtype must be None, torch.float32 or torch.bfloat16, got torch.int64"),
    ("tec-dtype-before-later-type", lambda: tec((), T.double(), None, TB),
     TypeError, "time_encode_cat computes in float32, t is torch.float64"),
    ("tec-t-rank-before-device", lambda: tec((), Z(4, 2), TW, M(3)),
     ValueError, "t must be [n] or [n, 1], got (4, 2)"),
    ("tec-weight-device-before-part-device", lambda: tec((M(4, 2),), T, M(3, 1), TB),
     ValueError, "weight is on meta, t on cpu"),

    # ---- edge_score
    ("es-type", lambda: es(SRC, None, W, BIAS),
     TypeError, "dst must be a tensor, got NoneType"),
    ("es-dtypes", lambda: es(SRC, DST.to(BF16), W, BIAS),
     TypeError, "edge_score computes in float32 and takes src and dst both float32 or both "
                "bfloat16, src is torch.float32 and dst is torch.bfloat16"),
    ("es-weight-dtype", lambda: es(SRC, DST, W.double(), BIAS),
     TypeError, "edge_score computes in float32, weight is torch.float64"),
    ("es-rank", lambda: es(SRC, Z(8, 3, 1), W, BIAS),
     ValueError, "src and dst must be [B, D] and [M, D], got (4, 3) and (8, 3, 1)"),
    ("es-columns", lambda: es(SRC, Z(8, 4), W, BIAS),
     ValueError, "src has 3 columns, dst has 4"),
    ("es-empty", lambda: es(Z(4, 0), Z(8, 0), Z(0), BIAS),
     ValueError, "edge_score needs D >= 1"),
    ("es-weight-shape", lambda: es(SRC, DST, Z(3, 1), BIAS),
     ValueError, "weight must be [D] or [1, D] with D = 3, got (3, 1)"),
    ("es-bias-shape", lambda: es(SRC, DST, W, Z(2)),
     ValueError, "bias must be [1], got (2,)"),
    ("es-rows", lambda: es(SRC, Z(7, 3), W, BIAS),
     ValueError, "dst has 7 rows, not a multiple of the 4 rows of src"),
    ("es-rows-no-src", lambda: es(Z(0, 3), DST, W, BIAS),
     ValueError, "dst has 8 rows, not a multiple of the 0 rows of src"),
    ("es-device", lambda: es(SRC, DST, M(1, 3), BIAS),
     ValueError, "weight is on meta, dst on cpu"),
    ("es-gpu", lambda: es(SRC, DST, W, BIAS),
     ValueError, "edge_score runs on the GPU, the inputs are on cpu"),
    ("es-dtypes-before-rank", lambda: es(Z(4, dtype=BF16), DST, W, BIAS),
     TypeError, "edge_score computes in float32 and takes src and dst both float32 or both "
                "bfloat16, src is torch.bfloat16 and dst is torch.float32"),
    ("es-type-before-dtypes", lambda: es(SRC.double(), DST, W, 0.0),
     TypeError, "bias must be a tensor, got float"),
    ("es-bias-shape-before-device", lambda: es(SRC, DST, M(3), Z(1, 1)),
     ValueError, "bias must be [1], got (1, 1)"),
    ("es-src-device-first", lambda: es(M(4, 3), DST, M(3), BIAS),
     ValueError, "src is on meta, dst on cpu"),

    # ---- edge_rank
    ("er-type", lambda: er(SRC, [CAND], W, BIAS),
     TypeError, "cand must be a tensor, got list"),
    ("er-int-type", lambda: er(SRC, CAND, W, BIAS, skip=3),
     TypeError, "skip must be a tensor, got int"),
    ("er-dtype", lambda: er(SRC, CAND, W, BIAS, ref_score=Z(4, dtype=F64)),
     TypeError, "edge_rank computes in float32, ref_score is torch.float64"),
    ("er-int-dtype", lambda: er(SRC, CAND, W, BIAS, exclude=Z(4, 1, dtype=I32)),
     TypeError, "exclude must be int64, got torch.int32"),
    ("er-k-type", lambda: er(SRC, CAND, W, BIAS, k=1.0),
     TypeError, "k must be an int, got float"),
    ("er-rank", lambda: er(SRC, Z(10), W, BIAS),
     ValueError, "src and cand must be [B, D] and [C, D], got (4, 3) and (10,)"),
    ("er-columns", lambda: er(SRC, Z(10, 2), W, BIAS),
     ValueError, "src has 3 columns, cand has 2"),
    ("er-empty", lambda: er(Z(4, 0), Z(10, 0), Z(0), BIAS),
     ValueError, "edge_rank needs D >= 1"),
    ("er-no-candidate", lambda: er(SRC, Z(0, 3), W, BIAS),
     ValueError, "edge_rank needs at least one candidate"),
    ("er-candidates", lambda: er(SRC, M(2 ** 31, 3), W, BIAS),
     ValueError, "edge_rank takes fewer than 2**31 candidates per call, got 2147483648"),
    ("er-weight-shape", lambda: er(SRC, CAND, Z(2, 3), BIAS),
     ValueError, "weight must be [D] or [1, D] with D = 3, got (2, 3)"),
    ("er-bias-shape", lambda: er(SRC, CAND, W, Z(())),
     ValueError, "bias must be [1], got ()"),
    ("er-k-range", lambda: er(SRC, CAND, W, BIAS, k=11),
     ValueError, "k must be in [0, min(C, 64)] with C = 10, got 11"),
    ("er-k-max", lambda: er(SRC, Z(100, 3), W, BIAS, k=65),
     ValueError, "k must be in [0, min(C, 64)] with C = 100, got 65"),
    ("er-ref-shape", lambda: er(SRC, CAND, W, BIAS, ref_score=Z(3)),
     ValueError, "ref_score must be [B] or [B, 1] with B = 4, got (3,)"),
    ("er-skip-shape", lambda: er(SRC, CAND, W, BIAS, skip=Z(4, 1, dtype=I64)),
     ValueError, "skip must be [B] with B = 4, got (4, 1)"),
    ("er-exclude-shape", lambda: er(SRC, Z(65, 3), W, BIAS, exclude=Z(4, 1, dtype=I64)),
     ValueError, "exclude must be [B, (C + 63) // 64] = [4, 2], got (4, 1)"),
    ("er-device", lambda: er(SRC, M(10, 3), W, BIAS),
     ValueError, "cand is on meta, src on cpu"),
    ("er-int-device", lambda: er(SRC, CAND, W, BIAS, k=1, skip=M(4, dtype=I64)),
     ValueError, "skip is on meta, src on cpu"),
    ("er-gpu", lambda: er(SRC, CAND, W, BIAS, k=2, ref_score=Z(4, 1)),
     ValueError, "edge_rank runs on the GPU, the inputs are on cpu"),
    ("er-k-type-before-rank", lambda: er(Z(4), CAND, W, BIAS, k=True),
     TypeError, "k must be an int, got bool"),
    ("er-dtype-before-int-dtype",
     lambda: er(SRC.double(), CAND, W, BIAS, skip=Z(4, dtype=I32)),
     TypeError, "edge_rank computes in float32, src is torch.float64"),
    ("er-int-type-before-dtype", lambda: er(SRC.double(), CAND, W, BIAS, exclude=[0]),
     TypeError, "exclude must be a tensor, got list"),
    ("er-k-range-before-device", lambda: er(SRC, M(10, 3), W, BIAS, k=-1),
     ValueError, "k must be in [0, min(C, 64)] with C = 10, got -1"),
    ("er-ref-device-before-skip-device",
     lambda: er(SRC, CAND, W, BIAS, ref_score=M(4), skip=M(4, dtype=I64)),
     ValueError, "ref_score is on meta, src on cpu"),

    # ---- dropout_relu_layer_norm
    ("drln-type", lambda: drln(X, G.numpy(), BE),
     TypeError, "weight must be a tensor, got ndarray"),
    ("drln-x-dtype", lambda: drln(X.half(), G, BE),
     TypeError, "dropout_relu_layer_norm computes in float32 and takes x float32 or bfloat16, "
                "x is torch.float16"),
    ("drln-dtype", lambda: drln(X.to(BF16), G, BE.to(BF16)),
     TypeError, "dropout_relu_layer_norm computes in float32, bias is torch.bfloat16"),
    ("drln-rank", lambda: drln(Z(4, 6, 1), G, BE),
     ValueError, "x must be [R, D], got (4, 6, 1)"),
    ("drln-empty", lambda: drln(Z(4, 0), Z(0), Z(0)),
     ValueError, "dropout_relu_layer_norm needs D >= 1"),
    ("drln-width", lambda: drln(Z(1, 1025), Z(1025), Z(1025)),
     ValueError, "D = 1025 exceeds LAYER_EPILOGUE_MAX_WIDTH (1024)"),
    ("drln-shape", lambda: drln(X, G, Z(1, 6)),
     ValueError, "bias must be [D] with D = 6, got (1, 6)"),
    ("drln-eps-zero", lambda: drln(X, G, BE, eps=0),
     ValueError, "eps must be > 0 in float32, got 0.0"),
    ("drln-eps-nan", lambda: drln(X, G, BE, eps=float("nan")),
     ValueError, "eps must be > 0 in float32, got nan"),
    ("drln-eps-underflows", lambda: drln(X, G, BE, eps=1e-60),
     ValueError, "eps must be > 0 in float32, got 1e-60"),
    ("drln-p-negative", lambda: drln(X, G, BE, dropout_p=-0.5),
     ValueError, P_RANGE.format("-0.5")),
    ("drln-p-nan", lambda: drln(X, G, BE, dropout_p=float("nan")),
     ValueError, P_RANGE.format("nan")),
    ("drln-p-one", lambda: drln(X, G, BE, dropout_p=1.0),
     ValueError, P_RANGE.format("1.0")),
    ("drln-p-rounds", lambda: drln(X, G, BE, dropout_p=ALMOST_ONE),
     ValueError, P_ROUNDS),
    ("drln-seed-range", lambda: drln(X, G, BE, dropout_p=0.5, dropout_seed=2 ** 64),
     ValueError, SEED_RANGE),
    ("drln-seed-range-without-dropout", lambda: drln(X, G, BE, dropout_seed=2 ** 64),
     ValueError, SEED_RANGE),
    ("drln-seed-defaults", lambda: drln(X, G, BE, dropout_p=0.5),
     ValueError, "dropout_relu_layer_norm runs on the GPU, the inputs are on cpu"),
    ("drln-device", lambda: drln(X, G, M(6)),
     ValueError, "bias is on meta, x on cpu"),
    ("drln-gpu", lambda: drln(X, G, BE),
     ValueError, "dropout_relu_layer_norm runs on the GPU, the inputs are on cpu"),
    ("drln-eps-before-p", lambda: drln(X, G, BE, eps=-1.0, dropout_p=2.0),
     ValueError, "eps must be > 0 in float32, got -1.0"),
    ("drln-shape-before-eps", lambda: drln(X, Z(5), BE, eps=0.0),
     ValueError, "weight must be [D] with D = 6, got (5,)"),
    ("drln-p-before-device", lambda: drln(X, M(6), BE, dropout_p=1.0),
     ValueError, P_RANGE.format("1.0")),
    ("drln-seed-before-device", lambda: drln(X, M(6), BE, dropout_seed=-1),
     ValueError, "dropout_seed must be in [0, 2**64), got -1"),
    ("drln-p-before-seed", lambda: drln(X, G, BE, dropout_p=ALMOST_ONE, dropout_seed=2 ** 64),
     ValueError, P_ROUNDS),

    # ---- gru_cell
    ("gru-type", lambda: gru(GI, GH.numpy(), HX),
     TypeError, "gh must be a tensor, got ndarray"),
    ("gru-residual-type", lambda: gru(GI, GH, HX, 1.0),
     TypeError, "residual must be a tensor or None, got float"),
    ("gru-num-last-type", lambda: gru(GI, GH, HX, None, 1.0),
     TypeError, "num_last must be an int, got float"),
    ("gru-dtypes", lambda: gru(GI, GH.to(BF16), HX),
     TypeError, "gru_cell computes in float32 and takes gi and gh both float32 or both "
                "bfloat16, gi is torch.float32 and gh is torch.bfloat16"),
    ("gru-hx-dtype", lambda: gru(GI.to(BF16), GH.to(BF16), HX.to(BF16)),
     TypeError, "gru_cell computes in float32, hx is torch.bfloat16"),
    ("gru-residual-dtype", lambda: gru(GI, GH, HX, HX.double()),
     TypeError, "gru_cell takes a float32 or bfloat16 residual, residual is torch.float64"),
    ("gru-rank", lambda: gru(GI, GH, Z(4, 3, 1)),
     ValueError, "hx must be [N, H], got (4, 3, 1)"),
    ("gru-empty", lambda: gru(Z(4, 0), Z(4, 0), Z(4, 0)),
     ValueError, "gru_cell needs H >= 1"),
    ("gru-shape", lambda: gru(GI, Z(4, 8), HX),
     ValueError, "gh must be [N, 3H] = [4, 9], got (4, 8)"),
    ("gru-residual-shape", lambda: gru(GI, GH, HX, Z(3, 3)),
     ValueError, "residual must be [N, H] = [4, 3], got (3, 3)"),
    ("gru-num-last-range", lambda: gru(GI, GH, HX, num_last=5),
     ValueError, "num_last must be in [0, 4], got 5"),
    ("gru-device", lambda: gru(GI, M(4, 9), HX),
     ValueError, "gh is on meta, hx on cpu"),
    ("gru-residual-device", lambda: gru(GI, GH, HX, M(4, 3, dtype=BF16)),
     ValueError, "residual is on meta, hx on cpu"),
    ("gru-gpu", lambda: gru(GI, GH, HX, HX, 4),
     ValueError, "gru_cell runs on the GPU, the inputs are on cpu"),
    ("gru-num-last-type-before-dtypes", lambda: gru(GI.double(), GH, HX, num_last=True),
     TypeError, "num_last must be an int, got bool"),
    ("gru-residual-type-before-num-last-type", lambda: gru(GI, GH, HX, [0.0], 1.0),
     TypeError, "residual must be a tensor or None, got list"),
    ("gru-num-last-range-before-device", lambda: gru(GI, M(4, 9), HX, num_last=-1),
     ValueError, "num_last must be in [0, 4], got -1"),
    ("gru-gi-shape-before-gh-shape", lambda: gru(Z(3, 9), Z(4, 8), HX),
     ValueError, "gi must be [N, 3H] = [4, 9], got (3, 9)"),

    # ---- link_metrics
    ("lm-type", lambda: lm(POS, [0.0]),
     TypeError, "neg must be a tensor, got list"),
    ("lm-dtype", lambda: lm(POS, NEG.double()),
     TypeError, "link_metrics ranks float32 scores, neg is torch.float64"),
    ("lm-rank", lambda: lm(Z(4, 2), NEG),
     ValueError, "pos must be [n] or [n, 1], got (4, 2)"),
    ("lm-empty", lambda: lm(POS, Z(0, 1)),
     ValueError, "link_metrics needs at least one positive and one negative score, got 4 and 0"),
    ("lm-scores", lambda: lm(POS, M(65533)),
     ValueError, "link_metrics takes at most 65536 scores per call, got 4 + 65533"),
    ("lm-device", lambda: lm(POS, M(8)),
     ValueError, "neg is on meta, pos on cpu"),
    ("lm-gpu", lambda: lm(POS, NEG),
     ValueError, "link_metrics runs on the GPU, the inputs are on cpu"),
    ("lm-gpu-before-accumulator", lambda: lm(POS, NEG, accumulator=[0.0] * 8),
     ValueError, "link_metrics runs on the GPU, the inputs are on cpu"),
    ("lm-pos-rank-before-neg-type", lambda: lm(Z(4, 2), None),
     ValueError, "pos must be [n] or [n, 1], got (4, 2)"),
    ("lm-pos-dtype-before-neg-type", lambda: lm(POS.to(BF16), None),
     TypeError, "link_metrics ranks float32 scores, pos is torch.bfloat16"),
    ("lm-empty-before-device", lambda: lm(Z(0), M(8)),
     ValueError, "link_metrics needs at least one positive and one negative score, got 0 and 8"),
    ("lm-scores-before-device", lambda: lm(POS, M(65536, 1)),
     ValueError, "link_metrics takes at most 65536 scores per call, got 4 + 65536"),

    # ---- link_loss
    ("ll-type", lambda: ll(3.0, NEG),
     TypeError, "pos must be a tensor, got float"),
    ("ll-dtypes", lambda: ll(POS, NEG.to(BF16)),
     TypeError, "link_loss computes in float32 and takes pos and neg both float32 or both "
                "bfloat16, pos is torch.float32 and neg is torch.bfloat16"),
    ("ll-rank", lambda: ll(POS, Z(8, 2)),
     ValueError, "neg must be [n] or [n, 1], got (8, 2)"),
    ("ll-empty", lambda: ll(Z(0, 1), NEG),
     ValueError, "link_loss needs at least one positive and one negative logit, got 0 and 8"),
    ("ll-logits", lambda: ll(POS, M(2 ** 31)),
     ValueError, "link_loss takes fewer than 2^31 logits on a side, got 4 and 2147483648"),
    ("ll-accumulator-type", lambda: ll(POS, NEG, [0.0] * 5),
     TypeError, "accumulator must be a tensor, got list"),
    ("ll-accumulator-dtype", lambda: ll(POS, NEG, Z(5)),
     TypeError, "accumulator must be float64, got torch.float32"),
    ("ll-accumulator-shape", lambda: ll(POS, NEG, Z(8, dtype=F64)),
     ValueError, "accumulator must be a contiguous [5] tensor, got (8,)"),
    ("ll-accumulator-strided", lambda: ll(POS, NEG, Z(10, dtype=F64)[::2]),
     ValueError, "accumulator must be a contiguous [5] tensor, got (5,)"),
    ("ll-device", lambda: ll(POS, M(8)),
     ValueError, "neg is on meta, pos on cpu"),
    ("ll-accumulator-device", lambda: ll(POS, NEG, M(5, dtype=F64)),
     ValueError, "accumulator is on meta, pos on cpu"),
    ("ll-gpu", lambda: ll(POS, NEG, Z(5, dtype=F64)),
     ValueError, "link_loss runs on the GPU, the inputs are on cpu"),
    ("ll-empty-before-accumulator", lambda: ll(Z(0), NEG, M(5)),
     ValueError, "link_loss needs at least one positive and one negative logit, got 0 and 8"),
    ("ll-accumulator-dtype-before-device", lambda: ll(POS, M(8), M(5)),
     TypeError, "accumulator must be float64, got torch.float32"),
    ("ll-accumulator-shape-before-device", lambda: ll(POS, M(8), Z(5, 1, dtype=F64)),
     ValueError, "accumulator must be a contiguous [5] tensor, got (5, 1)"),
    ("ll-device-before-accumulator-device", lambda: ll(POS, M(8), M(5, dtype=F64)),
     ValueError, "neg is on meta, pos on cpu"),
    ("ll-dtypes-before-rank", lambda: ll(Z(4, 2), NEG.double()),
     TypeError, "link_loss computes in float32 and takes pos and neg both float32 or both "
                "bfloat16, pos is torch.float32 and neg is torch.float64"),
    ("ll-neg-type-before-pos-rank", lambda: ll(Z(4, 2), None),
     TypeError, "neg must be a tensor, got NoneType"),

    # ---- walk_position_counts, check_walk_position_counts_args
    ("walk-type", lambda: wargs([[0]]),
     TypeError, "nodes must be a tensor, got list"),
    ("walk-dtype", lambda: wargs(NODES, NODES.to(I32)),
     TypeError, "ref must be torch.int64, got torch.int32"),
    ("walk-rank", lambda: wargs(Z(4, 3, dtype=I64)),
     ValueError, "nodes must be [rows, walks, length + 1], got shape (4, 3)"),
    ("walk-length", lambda: wargs(Z(2, 3, 34, dtype=I64)),
     ValueError, "nodes must hold walks of 0 to 32 steps (1 to 33 nodes), got 34 nodes"),
    ("walk-no-node", lambda: wargs(NODES, Z(2, 3, 0, dtype=I64)),
     ValueError, "ref must hold walks of 0 to 32 steps (1 to 33 nodes), got 0 nodes"),
    ("walk-rows", lambda: wargs(NODES, Z(3, 3, 5, dtype=I64)),
     ValueError, "nodes has 2 rows, ref has 3"),
    ("walk-entries", lambda: wargs(Z(1, 200, 33, dtype=I64)),
     ValueError, "walk_position_counts counts in at most 4096 entries per row, got 200 x 33"),
    ("walk-many-rows", lambda: wargs(M(2 ** 31, 1, 1, dtype=I64)),
     ValueError, "walk_position_counts takes fewer than 2**31 rows, got 2147483648"),
    ("walk-counts", lambda: wargs(M(1, 2000000, 33, dtype=I64), M(1, 1, 33, dtype=I64)),
     ValueError, "walk_position_counts writes fewer than 2**31 counts per row, got "
                 "2000000 x 33 x 33"),
    ("walk-device", lambda: wargs(NODES, M(2, 3, 5, dtype=I64)),
     ValueError, "ref is on meta, nodes on cpu"),
    ("walk-gpu", lambda: wpc(NODES),
     ValueError, "walk_position_counts runs on the GPU, the inputs are on cpu"),
    ("walk-gpu-with-ref", lambda: wpc(NODES, Z(2, 7, 2, dtype=I64)),
     ValueError, "walk_position_counts runs on the GPU, the inputs are on cpu"),
    ("walk-args-before-gpu", lambda: wpc(NODES.to(I32)),
     TypeError, "nodes must be torch.int64, got torch.int32"),
    ("walk-nodes-rank-before-ref-dtype", lambda: wpc(Z(4, 3, dtype=I64), NODES.to(I32)),
     ValueError, "nodes must be [rows, walks, length + 1], got shape (4, 3)"),
    ("walk-rows-before-device", lambda: wargs(NODES, M(3, 3, 5, dtype=I64)),
     ValueError, "nodes has 2 rows, ref has 3"),
    ("walk-entries-before-many-rows", lambda: wargs(M(2 ** 31, 200, 33, dtype=I64)),
     ValueError, "walk_position_counts counts in at most 4096 entries per row, got 200 x 33"),
]


@pytest.mark.parametrize("call, exc, message", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_error_contract(call, exc, message):
    with pytest.raises(exc) as info:
        call()
    assert type(info.value) is exc
    assert str(info.value) == message


def test_the_ids_are_distinct():
    assert len({c[0] for c in CASES}) == len(CASES)
