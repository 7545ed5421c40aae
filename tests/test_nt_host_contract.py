"""The host contract of the split-operand NT product, the part that needs no GPU: what the five entry points (tfgnn_sp_gemm_nt,
_sp, _dropout, _rows, _grouped) answer to the calls they reject - return code and the exact text of tfgnn_last_error.
tests/golden/nt_host_contract_parent.json is what ``contract()`` below returned at the commit before the 36-parameter host
function behind them became a call description (csrc/gemm_sp.hpp NtCall) and sp_nt_enqueue: ops.py raises with these texts,
INTEGRATION.md documents the codes, and binders from other frameworks match both.  Some texts name another entry point than
the one that was called (the checks are shared); that is part of the record.

Every call here returns before the library touches a device, so the pointers are arbitrary aligned non-null values.  Four
calls carry two faults each and pin that the first check, in the order of the parent commit, is the one that answers.

Exempt, because they need a device: "no device memory for this device's epoch word" (the dropout epoch word could not be
allocated) and the error a product call returns after a K-split reducer of an earlier product timed out."""
import json
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "nt_host_contract_parent.json"

A, INV_A, B, INV_B, C, BIAS, MUL, SAVED, OUT_SP, OUT_INV = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000, 0x90000, 0xA0000
A_ROWS, KMASK, ROW_MAP, TABLE = 0xB0000, 0xC0000, 0xD0000, 0xE0000
UNSUPPORTED = -4


def common(**over):
    """The arguments every entry point has, of a valid product [256, 64] x [128, 64]^T with one scale per row of A"""
    a = dict(M=256, N=128, K=64, A=A, lda=256, inv_a=INV_A, sb=0, B=B, ldb=256, inv_b=INV_B, C=C, ldc=128, bias=None, act=0,
             accumulate=0, mul=None, ld_mul=0, act_of_saved=0, saved=None, ld_saved=0, stream=None)
    a.update(over)
    return a


def nt_args(**over):
    a = common(**over)
    return tuple(a[k] for k in ("M", "N", "K", "A", "lda", "inv_a", "sb", "B", "ldb", "inv_b", "C", "ldc", "bias", "act", "accumulate",
                                "mul", "ld_mul", "act_of_saved", "saved", "ld_saved", "stream"))


def sp_args(**over):
    a = common(out_sp=OUT_SP, ld_out_sp=512, out_inv=OUT_INV)
    a.update(over)
    return tuple(a[k] for k in ("M", "N", "K", "A", "lda", "inv_a", "sb", "B", "ldb", "inv_b", "C", "ldc", "bias", "act", "mul", "ld_mul",
                                "act_of_saved", "saved", "ld_saved", "out_sp", "ld_out_sp", "out_inv", "stream"))


def rows_args(**over):
    """tfgnn_sp_gemm_nt_rows; tfgnn_sp_gemm_nt_dropout takes the same without a_rows"""
    a = common(a_rows=None, saved_scale=1.0, out_sp=None, ld_out_sp=0, out_inv=None, rate=0.0, seed=0, kmask=None, row_map=None)
    a.update(over)
    return tuple(a[k] for k in ("M", "N", "K", "A", "lda", "inv_a", "sb", "a_rows", "B", "ldb", "inv_b", "C", "ldc", "bias", "act",
                                "accumulate", "mul", "ld_mul", "act_of_saved", "saved", "ld_saved", "saved_scale", "out_sp", "ld_out_sp",
                                "out_inv", "rate", "seed", "kmask", "row_map", "stream"))


def grouped_args(**over):
    """Two row tiles in two groups, the weight operands of the groups back to back"""
    a = common(a_rows=None, a_src_rows=0, table=TABLE, tiles=2, groups=2, b_group_stride=-1, b_scale_group_stride=-1, out_sp=None,
               ld_out_sp=0, out_inv=None)
    a.update(over)
    return tuple(a[k] for k in ("M", "N", "K", "A", "lda", "inv_a", "sb", "a_rows", "a_src_rows", "table", "tiles", "groups", "B", "ldb",
                                "b_group_stride", "inv_b", "b_scale_group_stride", "C", "ldc", "bias", "act", "mul", "ld_mul",
                                "act_of_saved", "saved", "ld_saved", "out_sp", "ld_out_sp", "out_inv", "stream"))


SPLIT_RESULT = dict(C=None, out_sp=OUT_SP, ld_out_sp=512, out_inv=OUT_INV)

REJECTIONS = [
    # the wrappers' own first checks
    ("nt C null", "tfgnn_sp_gemm_nt", nt_args(C=None)),
    ("sp out_sp null", "tfgnn_sp_gemm_nt_sp", sp_args(out_sp=None)),
    ("grouped without a table", "tfgnn_sp_gemm_nt_grouped", grouped_args(table=None)),
    # the shared checks
    ("rows A null", "tfgnn_sp_gemm_nt_rows", rows_args(A=None)),
    ("rows both outputs null", "tfgnn_sp_gemm_nt_rows", rows_args(C=None)),
    ("rows M=0", "tfgnn_sp_gemm_nt_rows", rows_args(M=0)),
    ("rows K=40", "tfgnn_sp_gemm_nt_rows", rows_args(K=40)),
    ("rows N=96", "tfgnn_sp_gemm_nt_rows", rows_args(N=96)),
    ("rows lda_bytes=200", "tfgnn_sp_gemm_nt_rows", rows_args(lda=200)),
    ("rows ldc=130", "tfgnn_sp_gemm_nt_rows", rows_args(ldc=130)),
    ("rows d_mul off by 4 bytes", "tfgnn_sp_gemm_nt_rows", rows_args(mul=MUL + 4, ld_mul=128)),
    ("rows rate 1.0", "tfgnn_sp_gemm_nt_rows", rows_args(rate=1.0)),
    ("rows rate NaN", "tfgnn_sp_gemm_nt_rows", rows_args(rate=float("nan"))),
    ("rows a_scale_block=24", "tfgnn_sp_gemm_nt_rows", rows_args(sb=24)),
    ("rows tile mask with a tensor-wide scale", "tfgnn_sp_gemm_nt_rows", rows_args(kmask=KMASK, sb=-1)),
    ("rows tile mask over 16 blocks", "tfgnn_sp_gemm_nt_rows", rows_args(K=256, lda=1024, ldb=1024, sb=16, kmask=KMASK)),
    ("rows d_a_rows with an operand of 4 GB", "tfgnn_sp_gemm_nt_rows", rows_args(M=1 << 20, lda=4096, a_rows=A_ROWS)),
    ("rows K=2^22", "tfgnn_sp_gemm_nt_rows", rows_args(K=1 << 22, lda=1 << 24, ldb=1 << 24)),
    ("rows seed 2^64-1 at rate 0.5 without a saved tensor", "tfgnn_sp_gemm_nt_rows", rows_args(rate=0.5, seed=(1 << 64) - 1)),
    ("rows split result with accumulate", "tfgnn_sp_gemm_nt_rows", rows_args(**dict(SPLIT_RESULT, accumulate=1))),
    ("rows split result without its scale array", "tfgnn_sp_gemm_nt_rows", rows_args(**dict(SPLIT_RESULT, out_inv=None))),
    ("rows split result with ld_out_sp_bytes=500", "tfgnn_sp_gemm_nt_rows", rows_args(**dict(SPLIT_RESULT, ld_out_sp=500))),
    ("rows M=2^40", "tfgnn_sp_gemm_nt_rows", rows_args(M=1 << 40)),
    ("grouped b_group_stride_bytes=100", "tfgnn_sp_gemm_nt_grouped", grouped_args(b_group_stride=100)),
    # two faults each: the first check answers
    ("rows A null and K=40", "tfgnn_sp_gemm_nt_rows", rows_args(A=None, K=40)),
    ("rows K=40 and N=96", "tfgnn_sp_gemm_nt_rows", rows_args(K=40, N=96)),
    ("rows N=96 and lda_bytes=200", "tfgnn_sp_gemm_nt_rows", rows_args(N=96, lda=200)),
    ("grouped without a table and K=40", "tfgnn_sp_gemm_nt_grouped", grouped_args(table=None, K=40)),
]


def contract():
    """-> {case: [return code, error text]} of the library of THIS tree"""
    from tf2_gnn_amd import _lib

    lib = _lib.load()
    record = {}
    for name, fn, args in REJECTIONS:
        rc = getattr(lib, fn)(*args)
        record[name] = [rc, lib.tfgnn_last_error().decode("utf-8", "replace")]
    return record


def test_the_record_is_what_the_issue_lists():
    want = json.loads(GOLDEN.read_text())
    names = [name for name, _, _ in REJECTIONS]
    assert len(set(names)) == len(names) == 28 and sorted(want) == sorted(names)
    for name, (rc, text) in want.items():
        assert rc != 0 and text.startswith("tfgnn_sp_gemm_nt"), name
    # the tile width is the one unsupported shape; every other rejection is an invalid argument
    assert {name for name, (rc, _) in want.items() if rc == UNSUPPORTED} == {"rows N=96", "rows N=96 and lda_bytes=200"}
    assert len({rc for rc, _ in want.values()}) == 2
    # of two faults the earlier check answers
    for both, first in (("rows A null and K=40", "rows A null"), ("rows K=40 and N=96", "rows K=40"),
                        ("rows N=96 and lda_bytes=200", "rows N=96"), ("grouped without a table and K=40", "grouped without a table")):
        assert want[both] == want[first], both


def test_rejections_are_those_of_the_parent_commit():
    want = json.loads(GOLDEN.read_text())
    got = contract()
    differing = {k: (got.get(k), v) for k, v in want.items() if got.get(k) != v}
    assert not differing, differing
    assert got == want


if __name__ == "__main__":
    print(json.dumps(contract(), indent=1, sort_keys=True))
