"""How many workgroups should an NT launch give the weight-gradient reduce pass it carries (include/tfgnn.h tfgnn_tn_reduce_job)?
     python tools/nt_tail_reduce_probe.py [out.txt]
Times, with device events on one stream, the pair of products of one backward pass at the benchmark's two shapes:
  mp     dW [4, 320, 320] = X^T G over V = 30 000 rows (A columns 1280, 25 K ranges) beside the masked by-source input-gradient
         product G W^T (K = 1280, 235 row tiles holding 1 / 2 / 3 / 4 non-empty blocks in 91 / 26 / 28 / 90 tiles)
  dense  dW [320, 320] = H^T dZ over the same rows (83 K ranges) beside the unmasked input-gradient product dZ W^T (K = 320)
as   separate: TN product, reduce launch, NT product   (the stand-alone entries)
     carried:  TN product, NT product carrying the pass on B workgroups, B swept; B = lib is the library's own choice
Each variant runs ROUNDS rounds of REPS back-to-back pairs, variants alternating within a round; the figure is the median over
the rounds of (time of a round) / REPS, with the spread (max - min) next to it.  Results are checked bit for bit first."""
import statistics
import sys

import torch

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.dirname(__import__("os").path.abspath(__file__))))
from tf2_gnn_amd import ops  # noqa: E402

V, H, L = 30000, 320, 4
ROUNDS, REPS, WARM = 9, 40, 5
SWEEP = ("lib", 16, 32, 64, 128, 256, 512, 1024, 2048)


def shapes(dev):
    g = torch.Generator().manual_seed(1)
    tiles = (V + 127) // 128
    nblk = [1] * 91 + [2] * 26 + [3] * 28 + [4] * 90
    nblk = (nblk + [4] * tiles)[:tiles]
    G = torch.randn((V, L * H), generator=g) * 0.01
    mask = torch.zeros(tiles, dtype=torch.uint8)
    for t, n in enumerate(nblk):
        mask[t] = (1 << n) - 1
        G[t * 128:(t + 1) * 128, n * H:] = 0.0
    X = torch.randn((V, H), generator=g)
    W = torch.randn((L, H, H), generator=g) * 0.05
    ident = torch.arange(V, dtype=torch.int32, device=dev)
    saved = torch.relu(torch.randn((V, H), generator=g)).to(dev)
    g_sp = ops.sp_split_rows(G.to(dev), scale_block=H)
    x_sp = ops.sp_split_rows(X.to(dev))
    wh = ops.sp_split_rows(W.permute(1, 0, 2).reshape(H, L * H).contiguous().to(dev))
    dW = torch.empty((L, H, H), device=dev)
    mp = dict(tn=(g_sp, x_sp, dict(out=dW, scatter=(H, H * H, 1, H))),
              nt=(g_sp, wh, dict(act_grad=("relu", saved), tile_kmask=mask.to(dev), a_rows=ident, row_map=ident)))
    dZ = torch.randn((V, H), generator=g) * 0.01
    z_sp = ops.sp_split_rows(dZ.to(dev))
    wd = ops.sp_split_rows((torch.randn((H, H), generator=g) * 0.05).to(dev))
    dWd = torch.empty((H, H), device=dev)
    dense = dict(tn=(x_sp, z_sp, dict(out=dWd)), nt=(z_sp, wd, dict(act_grad=("relu", saved))))
    return {"mp": mp, "dense": dense}


def run(case, blocks, out_nt):
    a, b, kw = case["tn"]
    na, nb, nkw = case["nt"]
    if blocks is None:
        ops.sp_gemm_tn(a, b, **kw)
        return ops.sp_gemm_nt(na, nb, out=out_nt, **nkw)
    _, job = ops.sp_gemm_tn_product(a, b, **kw)
    if blocks != "lib":
        job.num_blocks = blocks
    return ops.sp_gemm_nt(na, nb, out=out_nt, tail=job, **nkw)


def main():
    dev = torch.device("cuda", 0)
    ops.set_gemm_mode("f16x2")
    lines = [f"TN product + reduce pass + NT product of one backward pass, V = {V}, H = {H}: us per pair, median of {ROUNDS} rounds of {REPS} "
             "(spread = max - min over the rounds)", ""]
    for name, case in shapes(dev).items():
        out_nt = torch.empty((V, H), device=dev)
        variants = [None] + list(SWEEP)
        want_nt = run(case, None, out_nt).clone()
        want_dw = case["tn"][2]["out"].clone()
        for v in variants[1:]:
            case["tn"][2]["out"].zero_()
            got = run(case, v, out_nt)
            torch.cuda.synchronize()
            assert torch.equal(got, want_nt) and torch.equal(case["tn"][2]["out"], want_dw), (name, v)
        times = {v: [] for v in variants}
        for v in variants:
            for _ in range(WARM):
                run(case, v, out_nt)
        torch.cuda.synchronize()
        for _ in range(ROUNDS):
            for v in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(REPS):
                    run(case, v, out_nt)
                e1.record()
                e1.synchronize()
                times[v].append(e0.elapsed_time(e1) * 1000.0 / REPS)
        rows, cols = case["tn"][2]["out"].numel() // H, H
        lib_blocks = max(1, min(1024, -(-rows * cols // 512)))
        lines.append(f"{name}: dW of {rows} x {cols} elements (library's count: {lib_blocks} workgroups); results bit-equal in every variant")
        for v in variants:
            t = times[v]
            label = "separate launches" if v is None else f"carried, {v} workgroups"
            lines.append(f"  {label:28s} {statistics.median(t):8.1f} us   spread {max(t) - min(t):5.1f}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text)


if __name__ == "__main__":
    main()
