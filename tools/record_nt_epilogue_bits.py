"""SHA-256 of every output of the split-operand NT product over small shapes that exercise its epilogue's row indexing: the
record that pins the product's results bit for bit across a change of how the epilogue fetches its row indices and its
gradient operands (csrc/gemm_sp.hip gemm_sp_nt_kernel).

    python tools/record_nt_epilogue_bits.py > tests/golden/nt_epilogue_parent_bits.json

Shapes: M in {1, 63, 130, 257} (the last row tile is partial, rows past the end clamp to the last row, at M = 1 / 130 / 257
whole waves own no valid row), N in {128, 256, 320} (the three tile widths), K in {32, 320} (two k16 steps - fewer than the
LDS ring holds - and twenty: no shape splits K inside its launch).  Routes: no row map; a random permutation as row map; the
by-source route (the same permutation as a_rows and row_map); both again with a tile mask over per-block scales (first tile
all-empty, second full, others partial).  Every route runs the forward and gradient epilogue forms of FORMS with plain output
and - but for the accumulating ones, which the split output excludes - with split output.  Grouped calls (tile table): groups of
1, 70 (ends inside the second wave's 64 rows), 0, 130 and 63 rows.  All inputs come from seeded host generators and the dropout
epoch is set to 0, so the hashes depend on the kernels alone.  tests/test_gpu_nt_epilogue_flight.py builds the same cases
through ``shapes()`` / ``run_shape()`` / ``run_grouped()`` and compares with the committed record.

A second shape list pins the products of the 320-column tile across a change of its wave geometry (eight waves of 32 x 160):

    python tools/record_nt_epilogue_bits.py eight-waves > tests/golden/nt_eight_waves_parent_bits.json

N = 320; M in {31, 32, 33, 96, 97, 127, 128, 129} (the 32-row boundaries of a wave and the tile edge); K in {16, 48, 80, 112,
320} (one k16 step, fewer steps than ring stages, odd and even step counts); the same routes and forms; grouped calls at
K = 48 and 320; and products at M = 257 that split K inside their launch in two (K = 480) and in four (K = 960), each
launched twice (``run_ksplit``).  tests/test_gpu_nt_eight_waves.py compares with that record."""
from __future__ import annotations

import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

M_SIZES = (1, 63, 130, 257)
N_SIZES = (128, 256, 320)
K_SIZES = (32, 320)
ROUTES = ("plain", "map", "map_rows", "mask_map", "mask_map_rows")
SCALE_BLOCK = {32: 16, 320: 80, 16: 16, 48: 16, 80: 16, 112: 16}  # masked routes: scale blocks that tile K (1 .. 7 of them)
EIGHT_WAVES = dict(m_sizes=(31, 32, 33, 96, 97, 127, 128, 129), n_sizes=(320,), k_sizes=(16, 48, 80, 112, 320))
EIGHT_WAVES_GROUPED_K = (48, 320)
KSPLIT_M, KSPLIT_N = 257, 320
KSPLIT_K = {2: 480, 4: 960}  # splits -> K (gemm_sp.hip: min(4, k16 steps / 15) splits while the grid fits the chip)
KSPLIT_FORMS = ("fwd", "both")
# name -> may also run with split output
FORMS = {"fwd": True, "fwd_bias_tanh_drop": True, "mul": True, "relu": True, "tanh09": True, "both": True, "acc": False,
         "acc_both": False, "drop": True, "drop_saved": True}
SAVED_SCALE = 0.9
FWD_DROP = (0.2, 77)
GRAD_DROP = (0.25, 9)
SAVED_DROP = (0.25, 5)
GROUP_SIZES = (1, 70, 0, 130, 63)
GROUPED_FORMS = ("relu_fwd_rows", "relu_grad", "tanh_grad_fp32")


def shapes(m_sizes=M_SIZES, n_sizes=N_SIZES, k_sizes=K_SIZES):
    """-> [(name, M, N, K, route)]"""
    return [(f"M{M} N{N} K{K} {route}", M, N, K, route) for M in m_sizes for N in n_sizes for K in k_sizes for route in ROUTES]


def grouped_shapes(n_sizes=N_SIZES, k_sizes=K_SIZES):
    return [(f"grouped N{N} K{K}", N, K) for N in n_sizes for K in k_sizes]


def ksplit_shapes():
    """-> [(name, M, N, K, "plain", splits)]: products that split K inside their launch"""
    return [(f"ksplit{S} M{KSPLIT_M} N{KSPLIT_N} K{K}", KSPLIT_M, KSPLIT_N, K, "plain", S) for S, K in KSPLIT_K.items()]


def tile_masks(M: int, K: int):
    """uint8 [row tiles]: the first tile all-empty and the second full where there are two; every other tile keeps its odd blocks"""
    nblk = K // SCALE_BLOCK[K]
    full = (1 << nblk) - 1
    tiles = (M + 127) // 128
    m = np.full(tiles, 0b1010 & full, dtype=np.uint8)
    if tiles >= 2:
        m[0], m[1] = 0, full
    return m


def host_inputs(shape):
    """seeded fp32 host tensors of one shape.  ``a_prod``: row r is what product row r multiplies; ``a``: the operand handed to
    the product (by-source routes: a[perm[r]] = a_prod[r]); ``dest``: output row of product row r"""
    import torch

    _, M, N, K, route = shape
    g = torch.Generator().manual_seed(100000 * ROUTES.index(route) + 1000 * M + N + K)
    a_prod = torch.randn((M, K), generator=g)
    bt = torch.randn((N, K), generator=g) * 0.05
    perm = torch.randperm(M, generator=g)
    masked = route.startswith("mask")
    kmask = None
    if masked:
        kmask = tile_masks(M, K)
        sb = SCALE_BLOCK[K]
        for t in range(kmask.size):
            for b in range(K // sb):
                if not (int(kmask[t]) >> b) & 1:
                    a_prod[t * 128:(t + 1) * 128, b * sb:(b + 1) * sb] = 0.0
    by_rows = route.endswith("rows")
    a = a_prod
    if by_rows:
        a = torch.empty_like(a_prod)
        a[perm] = a_prod
    saved = torch.tanh(torch.randn((M, N), generator=g))
    hidden = torch.relu(torch.randn((M, N), generator=g))
    keep = (torch.rand((M, N), generator=g) >= SAVED_DROP[0]).float() / (1.0 - SAVED_DROP[0])
    return dict(a=a, a_prod=a_prod, bt=bt, dest=(perm if route != "plain" else torch.arange(M)), by_rows=by_rows,
                kmask=None if kmask is None else torch.from_numpy(kmask), scale_block=SCALE_BLOCK[K] if masked else 0,
                bias=torch.randn(N, generator=g), mul=(torch.rand((M, N), generator=g) > 0.2).float() * 1.25, saved=saved,
                dropped=hidden * keep, base=torch.randn((M, N), generator=g))


def device_inputs(shape, dev):
    h = host_inputs(shape)
    d = {k: (v.to(dev) if hasattr(v, "to") else v) for k, v in h.items()}
    d["dest32"] = h["dest"].int().to(dev)
    return d


def form_kwargs(form: str, d, dev):
    """the epilogue arguments of ``ops.sp_gemm_nt`` / ``sp_gemm_nt_split`` for one form (device tensors of ``device_inputs``)"""
    from tf2_gnn_amd import ops

    M, N = d["mul"].shape
    return {
        "fwd": lambda: {},
        "fwd_bias_tanh_drop": lambda: dict(bias=d["bias"], act="tanh", dropout=FWD_DROP),
        "mul": lambda: dict(out_mul=d["mul"]),
        "relu": lambda: dict(act_grad=("relu", d["saved"])),
        "tanh09": lambda: dict(act_grad=("tanh", d["saved"]), saved_scale=SAVED_SCALE),
        "both": lambda: dict(out_mul=d["mul"], act_grad=("tanh", d["saved"])),
        "acc": lambda: dict(accumulate=True, out=d["base"].clone()),
        "acc_both": lambda: dict(accumulate=True, out=d["base"].clone(), out_mul=d["mul"], act_grad=("relu", d["saved"])),
        "drop": lambda: dict(act_grad=("relu", d["saved"]), dropout=GRAD_DROP),
        "drop_saved": lambda: dict(out_mul=ops.DropoutSpec(SAVED_DROP[0], SAVED_DROP[1], (M, N), dev),
                                   act_grad=("relu", d["dropped"], 1.0 - SAVED_DROP[0])),
    }[form]()


def run_shape(shape, dev, d=None):
    """every form of one shape -> {"<form> plain out" | "<form> split out" | "<form> split data" | "<form> split inv_scale": tensor}"""
    from tf2_gnn_amd import ops

    if d is None:
        d = device_inputs(shape, dev)
    route = shape[4]
    a_op = ops.sp_split_rows(d["a"], scale_block=d["scale_block"])
    b_op = ops.sp_split_rows(d["bt"])
    idx = {}
    if route != "plain":
        idx["row_map"] = d["dest32"]
    if d["by_rows"]:
        idx["a_rows"] = d["dest32"]
    if d["kmask"] is not None:
        idx["tile_kmask"] = d["kmask"]
    out = {}
    for form, splits in FORMS.items():
        out[f"{form} plain out"] = ops.sp_gemm_nt(a_op, b_op, **form_kwargs(form, d, dev), **idx)
        if splits:
            c, op = ops.sp_gemm_nt_split(a_op, b_op, **form_kwargs(form, d, dev), **idx)
            out[f"{form} split out"], out[f"{form} split data"], out[f"{form} split inv_scale"] = c, op.data, op.inv_scale
    return out


def grouped_host_inputs(shape):
    import torch

    _, N, K = shape
    R, G, V = sum(GROUP_SIZES), len(GROUP_SIZES), 90
    g = torch.Generator().manual_seed(7000 + N + K)
    return dict(x=torch.randn((V, K), generator=g), node=torch.randint(0, V, (R,), generator=g).int(),
                w=torch.randn((G, N, K), generator=g) * 0.05, a=torch.randn((R, K), generator=g),
                saved=torch.tanh(torch.randn((R, N), generator=g)))


def run_grouped(shape, dev, d=None):
    """the grouped product (tile table): rows through an index with relu and both outputs; relu' and tanh' of a saved tensor"""
    from tf2_gnn_amd import ops

    _, N, K = shape
    if d is None:
        d = {k: v.to(dev) for k, v in grouped_host_inputs(shape).items()}
    off = [0]
    for n in GROUP_SIZES:
        off.append(off[-1] + n)
    groups = ops.RowGroups(off, dev)
    w_op = ops.sp_split_rows(d["w"].reshape(len(GROUP_SIZES) * N, K))
    out = {}
    c, op = ops.sp_gemm_nt_grouped(ops.sp_split_rows(d["x"]), w_op, groups, a_rows=d["node"], act="relu", want_split=True)
    out["relu_fwd_rows out"], out["relu_fwd_rows data"], out["relu_fwd_rows inv_scale"] = c, op.data, op.inv_scale
    a_op = ops.sp_split_rows(d["a"])
    c, op = ops.sp_gemm_nt_grouped(a_op, w_op, groups, act_grad=("relu", d["saved"]), want_split=True)
    out["relu_grad out"], out["relu_grad data"], out["relu_grad inv_scale"] = c, op.data, op.inv_scale
    out["tanh_grad_fp32 out"], _ = ops.sp_gemm_nt_grouped(a_op, w_op, groups, act_grad=("tanh", d["saved"]))
    return out


def run_ksplit(shape, dev, d=None, after_launch=None):
    """KSPLIT_FORMS of one K-split shape, each launched twice back to back -> {"<form> first" | "<form> second": tensor}.
    ``after_launch(key)`` is called behind every launch (the test reads the split's flag words there)"""
    from tf2_gnn_amd import ops

    if d is None:
        d = device_inputs(shape[:5], dev)
    a_op = ops.sp_split_rows(d["a"])
    b_op = ops.sp_split_rows(d["bt"])
    out = {}
    for form in KSPLIT_FORMS:
        for turn in ("first", "second"):
            out[f"{form} {turn}"] = ops.sp_gemm_nt(a_op, b_op, **form_kwargs(form, d, dev))
            if after_launch is not None:
                after_launch(f"{form} {turn}")
    return out


def sha(tensors) -> str:
    """one hash over the bytes of several tensors, in the order given"""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def hashes(name: str, results) -> dict:
    """{"<shape> | <form>": hash over that form's arrays in the order run_shape / run_grouped made them}"""
    by_form = {}
    for key, t in results.items():
        by_form.setdefault(key.split(" ")[0], []).append(t)
    return {f"{name} | {form}": sha(ts) for form, ts in by_form.items()}


def record(dev, shape_list=None, grouped_list=None, ksplit_list=()):
    import torch

    from tf2_gnn_amd import ops

    ops.dropout_epoch_set(0)
    out = {}
    for shape in (shapes() if shape_list is None else shape_list):
        out.update(hashes(shape[0], run_shape(shape, dev)))
    for shape in (grouped_shapes() if grouped_list is None else grouped_list):
        out.update(hashes(shape[0], run_grouped(shape, dev)))
    for shape in ksplit_list:
        out.update(hashes(shape[0], run_ksplit(shape, dev)))
    torch.cuda.synchronize()
    return out


def eight_waves_lists():
    """-> (shapes, grouped shapes, K-split shapes) of the eight-waves record"""
    return shapes(**EIGHT_WAVES), grouped_shapes(EIGHT_WAVES["n_sizes"], EIGHT_WAVES_GROUPED_K), ksplit_shapes()


if __name__ == "__main__":
    import torch

    lists = eight_waves_lists() if sys.argv[1:] == ["eight-waves"] else ()
    print(json.dumps(record(torch.device("cuda", 0), *lists), indent=0, sort_keys=True))
