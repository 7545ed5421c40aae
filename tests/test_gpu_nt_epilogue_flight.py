"""The NT product's epilogue takes its output rows from one register per lane (loaded once per wave, handed round by a lane
exchange) and fetches the gradient operands of half a row tile in one flight (csrc/gemm_sp.hip gemm_sp_nt_kernel).  Arithmetic,
order of operations and stores did not change, so the checks are: bit-identity with the parent commit (recorded hashes), the
fp64 product behind every case, and a captured forward / backward pair replayed to the eager bits.

Cases: tools/record_nt_epilogue_bits.py (M in {1, 63, 130, 257} x N in {128, 256, 320} x K in {32, 320}; no row map, a row map,
the by-source route, both with a tile mask; forward and gradient epilogue forms with plain and split output; grouped calls).

Bounds (those tests/test_gpu_gemm_sp.py applies to the same product forms, |got - ref| <= tol * max(1, |ref|)):
  the bare product      1e-5 of max(1, 0.05 sqrt(K)) - which is 1 at K <= 400 (test_gemm_nt_matches_fp64)
  epilogue forms        2e-5 (test_gemm_nt_epilogues)
  grouped products      1e-5 (test_grouped_products_on_split_operands)
  split output          the fp32 result is the plain product's bit for bit and the SP16 form is the split of exactly those
                        values: same scales, same fp16 values (test_gemm_nt_split_result_equals_a_split_pass_over_the_fp32_result;
                        fp16 VALUES because act' makes zeros of either sign, test_grouped_products_on_split_operands)"""
import importlib.util
import json
from pathlib import Path

import pytest
import torch

from tests.helpers import assert_close, random_graph, to_dev

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
TOL_PRODUCT = 1e-5
TOL_EPILOGUE = 2e-5
TOL_GROUPED = 1e-5


def _load_recorder():
    spec = importlib.util.spec_from_file_location("record_nt_epilogue_bits", ROOT / "tools" / "record_nt_epilogue_bits.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


rec = _load_recorder()
SHAPES = rec.shapes()
GROUPED = rec.grouped_shapes()


@pytest.fixture(scope="module")
def golden():
    return json.loads((ROOT / "tests" / "golden" / "nt_epilogue_parent_bits.json").read_text())


@pytest.fixture(autouse=True)
def epoch_zero():
    from tf2_gnn_amd import ops

    ops.dropout_epoch_set(0)  # the recorded masks are those of epoch 0
    yield
    ops.dropout_epoch_set(0)


def _masks(shape, dev):
    from tf2_gnn_amd import ops

    M, N = shape[1], shape[2]
    return {seed: ops.dropout_mask((M, N), rate, seed, device=dev).cpu().double() for rate, seed in (rec.FWD_DROP, rec.GRAD_DROP)}


def _reference(form, h, masks):
    """fp64 value of one form in OUTPUT row order (product row r lands at row dest[r])"""
    prod = h["a_prod"].double() @ h["bt"].double().t()
    p = torch.zeros_like(prod)
    p[h["dest"]] = prod
    mul, saved, base = h["mul"].double(), h["saved"].double(), h["base"].double()
    relu_d = (saved > 0).double()
    if form == "fwd":
        return p
    if form == "fwd_bias_tanh_drop":
        return torch.tanh(p + h["bias"].double()) * masks[rec.FWD_DROP[1]]
    if form == "mul":
        return p * mul
    if form == "relu":
        return p * relu_d
    if form == "tanh09":
        return p * (1.0 - (rec.SAVED_SCALE * saved) ** 2)
    if form == "both":
        return p * mul * (1.0 - saved ** 2)
    if form == "acc":
        return p + base
    if form == "acc_both":
        return p * mul * relu_d + base
    if form == "drop":
        return p * relu_d * masks[rec.GRAD_DROP[1]]
    if form == "drop_saved":
        return p * (h["dropped"] > 0).double() / (1.0 - rec.SAVED_DROP[0])
    raise AssertionError(form)


def _check_split(name, out32, data, inv, bn):
    """the SP16 form is the split of exactly the fp32 values: same scales, same fp16 values"""
    from tf2_gnn_amd import ops

    ref = ops.sp_split_rows(out32, scale_block=bn)
    assert torch.equal(inv.view(-1), ref.inv_scale.view(-1)), f"{name}: row scales"
    assert torch.equal(data.view(torch.float16).float(), ref.data.view(torch.float16).float()), f"{name}: SP16 values"


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_shape_reproduces_the_parent_bits_and_the_fp64_product(dev, golden, shape):
    name, M, N, K, route = shape
    d = rec.device_inputs(shape, dev)
    res = rec.run_shape(shape, dev, d)
    torch.cuda.synchronize()
    got = rec.hashes(name, res)
    wrong = [k for k in got if golden.get(k) != got[k]]
    assert not wrong, wrong
    h = rec.host_inputs(shape)
    masks = _masks(shape, dev)
    for form, splits in rec.FORMS.items():
        ref = _reference(form, h, masks)
        plain = res[f"{form} plain out"]
        tol = TOL_PRODUCT if form == "fwd" else TOL_EPILOGUE
        assert_close(plain.cpu() / max(1.0, 0.05 * K ** 0.5), (ref / max(1.0, 0.05 * K ** 0.5)).float(), tol=tol, what=f"{name} {form}")
        if splits:
            assert torch.equal(res[f"{form} split out"], plain), f"{name} {form}: fp32 of the split form"
            _check_split(f"{name} {form}", plain, res[f"{form} split data"], res[f"{form} split inv_scale"], N)


@pytest.mark.parametrize("shape", GROUPED, ids=[s[0] for s in GROUPED])
def test_grouped_call_reproduces_the_parent_bits_and_the_fp64_product(dev, golden, shape):
    name, N, K = shape
    h = rec.grouped_host_inputs(shape)
    res = rec.run_grouped(shape, dev, {k: v.to(dev) for k, v in h.items()})
    torch.cuda.synchronize()
    got = rec.hashes(name, res)
    wrong = [k for k in got if golden.get(k) != got[k]]
    assert not wrong, wrong
    off = [0]
    for n in rec.GROUP_SIZES:
        off.append(off[-1] + n)
    w = h["w"].double()

    def per_group(rows):
        return torch.cat([rows[off[g]:off[g + 1]] @ w[g].t() for g in range(len(rec.GROUP_SIZES))])

    saved = h["saved"].double()
    refs = {"relu_fwd_rows": torch.relu(per_group(h["x"].double()[h["node"].long()])),
            "relu_grad": per_group(h["a"].double()) * (saved > 0).double(),
            "tanh_grad_fp32": per_group(h["a"].double()) * (1.0 - saved ** 2)}
    for form in rec.GROUPED_FORMS:
        assert_close(res[f"{form} out"].cpu(), refs[form].float(), tol=TOL_GROUPED, what=f"{name} {form}")
        if f"{form} data" in res:
            _check_split(f"{name} {form}", res[f"{form} out"], res[f"{form} data"], res[f"{form} inv_scale"], N)


def test_the_record_holds_exactly_these_cases(golden):
    want = {f"{s[0]} | {form}" for s in SHAPES for form in rec.FORMS} | {f"{s[0]} | {form}" for s in GROUPED for form in rec.GROUPED_FORMS}
    assert set(golden) == want


def test_captured_forward_backward_pair_replays_to_the_eager_bits(dev):
    """a 2-layer RGCN stack at V = 2500, H = 320 in f16x2 mode (masked forward products, by-source input-gradient products with
    relu' and accumulation): one forward / backward pair captured into a hipGraph, replayed twice, both equal to the eager run"""
    import bench
    from tf2_gnn_amd import CapturedStep, ops
    from tf2_gnn_amd.layers import GNN, GNNInput
    from tf2_gnn_amd.layers.message_passing import set_seed

    V, E, L, H = 2500, 60000, 4, 320
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode("f16x2")
    try:
        set_seed(0)
        gnn = GNN(bench.model_params("rgcn", H, 2, None))
        gen = torch.Generator().manual_seed(5)
        X = torch.randn((V, H), generator=gen).to(dev)
        dOut = torch.randn((V, H), generator=gen).to(dev)
        graph = ops.Graph(to_dev(random_graph(V, E, L, seed=3, hub=(5, 300)), dev), V, parts=ops.G_PARTS_ALL)
        inp = GNNInput(X, graph, torch.zeros(V, dtype=torch.int32, device=dev), 1)

        def step():
            gnn._dropout_calls = 0
            out = gnn(inp, training=False)
            dx = gnn.backward(dOut, need_input_grad=True)
            return [out, dx] + [v.grad for v in gnn.trainable_variables]

        def snapshot(res):
            torch.cuda.synchronize()
            return [t.clone() for t in res]

        eager = snapshot(step())
        cap = CapturedStep(step)
        cap.capture()
        for _ in range(2):
            replayed = snapshot(cap.replay())
            assert len(replayed) == len(eager)
            for a, b in zip(replayed, eager):
                assert torch.equal(a, b)
        assert not cap.guard_tripped()
        graph.close()
    finally:
        ops.set_gemm_mode(prev)
