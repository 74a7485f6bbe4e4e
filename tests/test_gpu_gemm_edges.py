"""The dense linear GEMMs' fused epilogues, element-wise, on ragged tiles and on
every tile class, epilogue kind and staging form launch_gemm can choose.

Every case names the kernel it means to reach -- (tile class, epilogue kind,
staging) as hvit_gemm_plan reports them -- and asserts that plan before it
launches, so a change to auto_tile or to the full-tile conditions that moves a
shape onto another kernel fails here instead of silently losing the cell
(test_case_plans does the same without a GPU, test_matrix_covers_every_cell
checks the matrix as a whole).

Reference: one float64 restatement of the epilogue in the order of the comment
above hvit_epilogue_t (include/hvit.h), applied to x.double() @ w.double().T of
the operands the kernel sees; the dropout mask is conftest.keep_mask at index
m * N + n.  Bars are test_gpu_bf16_exact.py's, element-wise: f32 outputs
|d| <= ACC max|ref|, bf16 outputs half a bf16 ulp more, acc = 1e-4 where GELU or
its derivative is evaluated, weight gradients 1e-4, tanh at ACC
(test_gpu_inference_kernels.py).  Dropout zeros are exact.

Every output (y, out2, the colsum rows, dw, db) lies inside a larger NaN buffer
with at least a 128-row tile of sentinel on either side: the bands must come
back bit for bit, and every element between them finite.

Shapes, from auto_tile's rules (csrc/gemm.h):
  64x64    anything small
  128x64   N <= 64 and ceil(M / 128) >= 160 (M = 20480; 20400 and 20440 ragged,
           the last tile's second 64-row half empty / partly empty), and
           N = 192 with ceil(M / 128) * 3 >= 160 (M = 6912; 6900 ragged)
  128x128  N = 1024, M = 2560 (160 tiles); 2500 and N = 1000 ragged
Each class also runs N % 4 != 0 (N = 5 / 6 / 7 / 10, 1001 / 1002): a partial
column group per thread, the per-element dropout hash of an odd m * N + n, and
column-sum rows that end inside a thread's four columns.  The weight gradient's
forced 128x128 tile runs with 40 and 104 output rows.
Staging: bf16 interior shapes take LDS-DMA -- one buffer on 128x128 plain store
and GELU_DUAL, three from K = 512 on the smaller tiles, else two -- everything
ragged and all f32 the register loop."""

import ctypes

import pytest
import torch

from conftest import keep_mask
from test_gpu_bf16_exact import ACC, check_bf16, check_f32

DEV = "cuda"
BF = torch.bfloat16
NAN = float("nan")
F32, BF16 = 0, 1
FWD, DGRAD, WGRAD = 0, 1, 2  # hvit_gemm_plan entries
A_NONE, A_DUAL, A_TANH, A_BWD, A_DUAL_D, A_MUL_AUX, A_GELU, A_DUAL_DK = 0, 1, 2, 3, 4, 5, 7, 9
GEN, STORE, SLAB, K_DUAL, K_RESID, K_BWD = 0, 1, 2, 3, 4, 5  # EpiKind
P_DROP, SEED, SITE = 0.1, 31, 411
RPS = 48      # rows per sample: divides none of the M below
RA_ROWS = 7   # rowadd period, likewise
BAND_ROWS = 128

# epilogue name -> what hvit_epilogue_t carries (bias: hvit_linear_fwd's argument)
EPIS = {
    "bias": dict(bias=1),
    "rowadd": dict(bias=1, rowadd=1),
    "dual": dict(act=A_DUAL, bias=1, drop=1, out2=1),
    "dual_d": dict(act=A_DUAL_D, bias=1, drop=1, out2=1),
    "dual_dk": dict(act=A_DUAL_DK, bias=1, drop=1, out2=1),
    "gelu": dict(act=A_GELU, bias=1, drop=1),
    "tanh": dict(act=A_TANH, bias=1),
    "tanh_drop": dict(act=A_TANH, bias=1, drop=1),
    "drop": dict(bias=1, drop=1),
    "resid_rs_drop": dict(bias=1, resid=1, rowscale=1, drop=1),
    "resid": dict(bias=1, resid=1),
    "bias_cs": dict(bias=1, colsum=1),
    "resid_rs_drop_cs": dict(bias=1, resid=1, rowscale=1, drop=1, colsum=1),
    "plain": dict(),
    "gelu_bwd_drop_cs": dict(act=A_BWD, aux=1, drop=1, colsum=1),
    "mul_aux_cs": dict(act=A_MUL_AUX, aux=1, colsum=1),
    "mul_aux_drop_cs": dict(act=A_MUL_AUX, aux=1, drop=1, colsum=1),
}
GELU_EPIS = {"dual", "dual_d", "dual_dk", "gelu", "gelu_bwd_drop_cs"}


class Case:
    """One launch: entry (FWD: y[M, NO] = x[M, KR] w[NO, KR]^T; DGRAD: dx[M, NO] =
    dy[M, KR] w[KR, NO]), operand and output types, the epilogue, the plan it must
    take, and `off`: the pointer handed over one element past 16-byte alignment."""

    def __init__(self, entry, dt, odt, M, NO, KR, epi, tile, ek, stage, why="", off=None):
        self.entry, self.dt, self.odt, self.M, self.NO, self.KR = entry, dt, odt, M, NO, KR
        self.epi, self.plan, self.why, self.off = epi, (0, tile, ek, stage), why, off
        self.id = "-".join(filter(None, [
            "fwd" if entry == FWD else "dgrad", f"{dt}to{odt}", f"{M}x{NO}x{KR}", epi, f"t{tile}k{ek}s{stage}", why,
            f"off_{off}" if off else None]))

    def api_nk(self):
        """(N, K) as the entry point names them."""
        return (self.NO, self.KR) if self.entry == FWD else (self.KR, self.NO)


def cases():
    c = []

    def fwd(dt, odt, M, NO, KR, epi, tile, ek, stage, why="", off=None):
        c.append(Case(FWD, dt, odt, M, NO, KR, epi, tile, ek, stage, why, off))

    def dgr(dt, odt, M, NO, KR, epi, tile, ek, stage, why="", off=None):
        c.append(Case(DGRAD, dt, odt, M, NO, KR, epi, tile, ek, stage, why, off))

    # ---- 64x64, both edges ragged (100 = 64 + 36 rows, 72 = 64 + 8 columns): every epilogue
    fwd("bf16", "bf16", 100, 72, 72, "bias", 64, STORE, 0, "raggedMN")
    fwd("f32", "f32", 100, 72, 72, "rowadd", 64, GEN, 0, "raggedMN")
    fwd("bf16", "bf16", 100, 72, 72, "dual", 64, GEN, 0, "raggedMN")
    fwd("f32", "f32", 100, 72, 72, "dual_d", 64, GEN, 0, "raggedMN")
    fwd("bf16", "f32", 100, 72, 72, "dual_dk", 64, GEN, 0, "raggedMN")
    fwd("bf16", "bf16", 100, 72, 72, "gelu", 64, GEN, 0, "raggedMN")
    fwd("f32", "f32", 100, 72, 72, "tanh_drop", 64, GEN, 0, "raggedMN")
    fwd("bf16", "f32", 100, 72, 72, "drop", 64, GEN, 0, "raggedMN")
    fwd("bf16", "f32", 100, 72, 72, "resid_rs_drop", 64, GEN, 0, "raggedMN")
    fwd("f32", "bf16", 100, 72, 72, "resid", 64, GEN, 0, "raggedMN")
    dgr("bf16", "bf16", 100, 72, 72, "gelu_bwd_drop_cs", 64, GEN, 0, "raggedMK")
    dgr("f32", "f32", 100, 72, 72, "mul_aux_cs", 64, GEN, 0, "raggedMK")
    dgr("bf16", "f32", 100, 72, 72, "plain", 64, STORE, 0, "raggedMK")
    # one edge only
    fwd("bf16", "bf16", 100, 64, 64, "resid_rs_drop", 64, GEN, 0, "raggedM")
    fwd("f32", "f32", 100, 64, 64, "bias", 64, STORE, 0, "raggedM")
    fwd("bf16", "bf16", 128, 72, 64, "dual_dk", 64, GEN, 0, "raggedN")
    fwd("f32", "f32", 128, 72, 64, "tanh", 64, GEN, 0, "raggedN")
    # the model's token counts at B = 1
    dgr("bf16", "bf16", 240, 72, 64, "mul_aux_drop_cs", 64, GEN, 0, "M240_raggedK")
    dgr("bf16", "bf16", 228, 128, 64, "gelu_bwd_drop_cs", 64, GEN, 0, "M228")
    dgr("bf16", "bf16", 240, 128, 64, "mul_aux_cs", 64, GEN, 0, "M240")
    # fewer rows than one 64-row half
    fwd("f32", "f32", 5, 24, 16, "resid_rs_drop", 64, GEN, 0, "M5")
    fwd("bf16", "bf16", 5, 24, 16, "bias", 64, STORE, 0, "M5")
    dgr("f32", "f32", 5, 24, 16, "mul_aux_cs", 64, GEN, 0, "M5")
    # N % 4 != 0: vec_ok false, nv < 4; an odd N makes m * N + n odd (the per-element hash)
    fwd("f32", "f32", 100, 5, 20, "drop", 64, GEN, 0, "N5_oddhash")
    fwd("f32", "f32", 100, 5, 20, "tanh_drop", 64, GEN, 0, "N5_oddhash")
    fwd("f32", "f32", 100, 6, 20, "bias", 64, GEN, 0, "N6")
    fwd("bf16", "f32", 100, 6, 24, "resid_rs_drop", 64, GEN, 0, "N6")
    fwd("bf16", "bf16", 100, 10, 24, "dual", 64, GEN, 0, "N10")
    fwd("bf16", "bf16", 100, 7, 24, "drop", 64, GEN, 0, "N7_oddhash")
    # ... with column sums: the column-sum rows end inside a thread's four columns
    fwd("f32", "f32", 100, 5, 20, "bias_cs", 64, GEN, 0, "N5_colsumtail")
    fwd("bf16", "f32", 100, 6, 24, "resid_rs_drop_cs", 64, GEN, 0, "N6_colsumtail")
    fwd("bf16", "f32", 100, 7, 24, "resid_rs_drop_cs", 64, GEN, 0, "N7_oddhash_colsumtail")
    # column sums of the forward kinds on full tiles: plain store keeps them, the residual
    # takes the generic kind (gemm_kernel's EK_RESID rows keep none)
    fwd("bf16", "bf16", 128, 128, 64, "bias_cs", 64, STORE, 2, "full_colsum")
    fwd("f32", "f32", 128, 128, 64, "resid_rs_drop_cs", 64, GEN, 0, "full_colsum")
    fwd("bf16", "f32", 128, 128, 64, "resid_rs_drop_cs", 64, GEN, 2, "full_colsum")
    # full 64x64 tiles: the compile-time kinds, two and three stage buffers, registers (f32, K % 64)
    fwd("bf16", "bf16", 128, 128, 64, "bias", 64, STORE, 2, "full")
    fwd("bf16", "bf16", 128, 128, 512, "dual", 64, K_DUAL, 3, "full")
    fwd("bf16", "f32", 128, 128, 64, "dual", 64, K_DUAL, 0, "full_f32out")
    fwd("bf16", "f32", 128, 128, 64, "resid_rs_drop", 64, K_RESID, 2, "full")
    fwd("bf16", "bf16", 128, 128, 64, "tanh_drop", 64, GEN, 2, "full")
    fwd("bf16", "bf16", 128, 128, 64, "gelu", 64, K_DUAL, 2, "full")
    fwd("bf16", "bf16", 128, 128, 72, "bias", 64, STORE, 0, "full_K72")
    fwd("f32", "f32", 128, 128, 64, "dual_dk", 64, K_DUAL, 0, "full")
    fwd("f32", "f32", 128, 128, 32, "resid", 64, K_RESID, 0, "full")
    dgr("bf16", "bf16", 128, 128, 64, "gelu_bwd_drop_cs", 64, K_BWD, 2, "full")
    dgr("bf16", "bf16", 128, 128, 512, "mul_aux_cs", 64, K_BWD, 3, "full")
    dgr("f32", "f32", 128, 128, 64, "gelu_bwd_drop_cs", 64, K_BWD, 0, "full")
    dgr("bf16", "f32", 128, 128, 64, "plain", 64, STORE, 2, "full")
    # a pointer one element off 16 bytes: the predicated rows, the result unchanged
    fwd("bf16", "bf16", 128, 128, 64, "bias", 64, GEN, 2, "full", off="y")
    fwd("bf16", "f32", 128, 128, 64, "resid_rs_drop", 64, GEN, 2, "full", off="resid")
    fwd("bf16", "bf16", 128, 128, 64, "dual", 64, GEN, 2, "full", off="out2")
    dgr("bf16", "bf16", 128, 128, 64, "gelu_bwd_drop_cs", 64, GEN, 2, "full", off="aux")

    # ---- 128x64 by the narrow rule
    fwd("bf16", "bf16", 20480, 64, 64, "bias", 12864, STORE, 2, "full")
    fwd("bf16", "bf16", 20480, 64, 512, "dual_dk", 12864, K_DUAL, 3, "full")
    fwd("bf16", "f32", 20480, 64, 64, "resid_rs_drop", 12864, K_RESID, 2, "full")
    fwd("bf16", "bf16", 20480, 64, 64, "drop", 12864, GEN, 2, "full")
    fwd("f32", "f32", 20480, 64, 64, "dual", 12864, K_DUAL, 0, "full")
    dgr("bf16", "bf16", 20480, 64, 64, "gelu_bwd_drop_cs", 12864, K_BWD, 2, "full")
    fwd("bf16", "bf16", 20400, 64, 64, "bias", 12864, STORE, 0, "raggedM_half2empty")
    fwd("bf16", "f32", 20440, 64, 64, "resid_rs_drop", 12864, GEN, 0, "raggedM_half2partly")
    fwd("bf16", "bf16", 20480, 40, 64, "dual", 12864, GEN, 0, "raggedN")
    fwd("bf16", "bf16", 20480, 40, 64, "bias", 12864, STORE, 0, "raggedN")
    fwd("f32", "f32", 20400, 40, 64, "tanh_drop", 12864, GEN, 0, "raggedMN")
    fwd("bf16", "bf16", 20440, 40, 64, "rowadd", 12864, GEN, 0, "raggedMN")
    dgr("bf16", "bf16", 20440, 40, 64, "mul_aux_drop_cs", 12864, GEN, 0, "raggedMK_half2partly")
    dgr("bf16", "bf16", 20400, 64, 64, "gelu_bwd_drop_cs", 12864, GEN, 0, "raggedM_half2empty")
    # N % 4 != 0 on the 128-row tile (RSTEP = 16 rows per sweep, two halves): nv < 4, the odd-index
    # hash, the column-sum rows ending inside a thread's four columns
    fwd("bf16", "f32", 20480, 6, 24, "resid_rs_drop", 12864, GEN, 0, "raggedN_N6")
    fwd("bf16", "bf16", 20480, 7, 24, "drop", 12864, GEN, 0, "raggedN_N7_oddhash")
    fwd("f32", "f32", 20440, 6, 24, "bias_cs", 12864, GEN, 0, "raggedMN_N6_colsumtail")
    fwd("bf16", "f32", 20440, 7, 24, "resid_rs_drop_cs", 12864, GEN, 0, "raggedMN_N7_oddhash_colsumtail")
    # ---- 128x64 by the half-empty-column rule (N = 192)
    fwd("bf16", "bf16", 6912, 192, 64, "dual", 12864, K_DUAL, 2, "full")
    fwd("bf16", "f32", 6912, 192, 64, "resid_rs_drop", 12864, K_RESID, 2, "full")
    fwd("bf16", "bf16", 6912, 192, 64, "bias", 12864, STORE, 2, "full")
    fwd("bf16", "f32", 6912, 192, 64, "tanh", 12864, GEN, 2, "full")
    dgr("bf16", "bf16", 6912, 192, 64, "mul_aux_drop_cs", 12864, K_BWD, 2, "full")
    fwd("bf16", "bf16", 6900, 192, 64, "dual_dk", 12864, GEN, 0, "raggedM")
    fwd("bf16", "bf16", 6900, 192, 64, "bias", 12864, STORE, 0, "raggedM")
    fwd("bf16", "f32", 6900, 192, 64, "resid_rs_drop", 12864, GEN, 0, "raggedM")
    dgr("bf16", "bf16", 6900, 192, 64, "mul_aux_cs", 12864, GEN, 0, "raggedM")

    # ---- 128x128
    fwd("bf16", "bf16", 2560, 1024, 64, "bias", 128, STORE, 1, "full")
    fwd("bf16", "bf16", 2560, 1024, 512, "dual", 128, K_DUAL, 1, "full")
    fwd("bf16", "f32", 2560, 1024, 64, "dual", 128, K_DUAL, 0, "full_f32out")
    fwd("bf16", "f32", 2560, 1024, 64, "resid_rs_drop", 128, K_RESID, 2, "full")
    fwd("bf16", "bf16", 2560, 1024, 64, "tanh_drop", 128, GEN, 2, "full")
    fwd("f32", "f32", 2560, 1024, 32, "dual_d", 128, K_DUAL, 0, "full")
    dgr("bf16", "bf16", 2560, 1024, 64, "gelu_bwd_drop_cs", 128, K_BWD, 2, "full")
    fwd("bf16", "bf16", 2500, 1024, 64, "bias", 128, STORE, 0, "raggedM_half2partly")
    fwd("bf16", "f32", 2500, 1024, 64, "resid_rs_drop", 128, GEN, 0, "raggedM")
    fwd("bf16", "bf16", 2560, 1000, 64, "dual_dk", 128, GEN, 0, "raggedN")
    fwd("bf16", "bf16", 2560, 1000, 64, "bias", 128, STORE, 0, "raggedN")
    fwd("f32", "f32", 2500, 1000, 64, "tanh_drop", 128, GEN, 0, "raggedMN")
    fwd("bf16", "bf16", 2500, 1000, 64, "rowadd", 128, GEN, 0, "raggedMN")
    dgr("bf16", "bf16", 2500, 1000, 64, "gelu_bwd_drop_cs", 128, GEN, 0, "raggedMK_half2partly")
    dgr("bf16", "f32", 2500, 1024, 64, "mul_aux_cs", 128, GEN, 0, "raggedM")
    # N % 4 != 0 on the 128x128 tile (RSTEP = 8): as above
    fwd("bf16", "bf16", 2560, 1002, 64, "dual", 128, GEN, 0, "raggedN_N1002")
    fwd("bf16", "f32", 2560, 1001, 64, "drop", 128, GEN, 0, "raggedN_N1001_oddhash")
    fwd("f32", "f32", 2500, 1001, 64, "tanh_drop", 128, GEN, 0, "raggedMN_N1001_oddhash")
    fwd("bf16", "f32", 2500, 1002, 64, "bias_cs", 128, GEN, 0, "raggedMN_N1002_colsumtail")
    fwd("bf16", "f32", 2500, 1001, 64, "resid_rs_drop_cs", 128, GEN, 0, "raggedMN_N1001_oddhash_colsumtail")
    fwd("bf16", "bf16", 2560, 1024, 64, "bias", 128, GEN, 2, "full", off="y")
    fwd("bf16", "f32", 2560, 1024, 64, "resid", 128, GEN, 2, "full", off="resid")
    fwd("bf16", "bf16", 2560, 1024, 64, "dual_d", 128, GEN, 2, "full", off="out2")
    dgr("bf16", "bf16", 2560, 1024, 64, "mul_aux_drop_cs", 128, GEN, 2, "full", off="aux")
    return c


CASES = cases()
# hvit_linear_wgrad at M = 1000, K = 24, N = 40 and 104: ragged on both output edges of the forced
# 128x128 tile, whose rows are the N outputs (40: less than one 64-row half; 104: the second half
# partly empty); three K slices by wgrad_splits with the last one short (1000 = 2 * 384 + 232 for
# bf16, 2 * 352 + 296 for f32), or one slice without a workspace.
# (N, dt, bias form, workspace, epilogue kind, splits)
WG_M, WG_NS, WG_K = 1000, (40, 104), 24
WGRAD_CASES = [(n, dt, db, ws, SLAB if ws else STORE, 3 if ws else 1)
               for n in WG_NS for dt in ("bf16", "f32") for db in ("none", "fused", "separate") for ws in (True, False)]


def tdt(name):
    return torch.float32 if name == "f32" else BF


def dtc(name):
    return F32 if name == "f32" else BF16


def esize(name):
    return 4 if name == "f32" else 2


def make_epi(L, c, ptrs):
    """hvit_epilogue_t of case c over ptrs: name -> (address, dtype name)."""
    spec = EPIS[c.epi]
    if not (set(spec) - {"bias"}):
        return None
    e = L.Epilogue()
    e.act = spec.get("act", A_NONE)
    if "out2" in spec:
        e.out2, e.out2_dt = ptrs["out2"][0], dtc(ptrs["out2"][1])
    if "aux" in spec:
        e.aux, e.aux_dt = ptrs["aux"][0], dtc(ptrs["aux"][1])
    e.dropout = L.dropout(P_DROP, SEED, SITE) if "drop" in spec else L.dropout()
    if "resid" in spec:
        e.resid = ptrs["resid"][0]
    if "rowscale" in spec:
        e.rowscale = ptrs["rowscale"][0]
    e.rows_per_sample = RPS
    if "rowadd" in spec:
        e.rowadd = ptrs["rowadd"][0]
    e.rowadd_rows = RA_ROWS
    if "colsum" in spec:
        e.colsum = ptrs["colsum"][0]
    return e


def query(L, c, ptrs):
    N, K = c.api_nk()
    p = L.GemmPlan()
    bias = ptrs["bias"][0] if (c.entry == FWD and "bias" in EPIS[c.epi]) else None
    L.call("hvit_gemm_plan", c.entry, dtc(c.dt), c.M, N, K, bias, ptrs["y"][0], dtc(c.odt), make_epi(L, c, ptrs), 0,
           ctypes.byref(p))
    return p.astuple()


@pytest.fixture()
def gemm_h_only(hv):
    """csrc/gemm.h's kernels only (the ring knob at 0), restored afterwards."""
    old = hv._lib.lib().hvit_gemm_tune(0, 0)
    yield lambda v: hv._lib.lib().hvit_gemm_tune(0, v)
    hv._lib.lib().hvit_gemm_tune(0, old)


# ------------------------------------------------------------------ no GPU ---
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_case_plans(hv, gemm_h_only, c):
    """Each case's plan from made-up addresses of the case's alignment: the matrix is
    checked where no GPU is."""
    L = hv._lib
    names = ["y", "out2", "aux", "resid", "rowscale", "rowadd", "colsum", "bias"]
    dts = {"y": c.odt, "out2": c.odt, "aux": c.dt}
    ptrs = {n: (0x100000 * (i + 1) + (esize(dts.get(n, "f32")) if c.off == n else 0), dts.get(n, "f32"))
            for i, n in enumerate(names)}
    assert query(L, c, ptrs) == c.plan


def test_matrix_covers_every_cell():
    plans = [c.plan for c in CASES]
    assert {p[1] for p in plans} == {64, 12864, 128}
    # every EpiKind the dense linear entries reach (EK_PATCH is the patch embedding's)
    assert {p[2] for p in plans} | {k for _, _, _, _, k, _ in WGRAD_CASES} == {GEN, STORE, SLAB, K_DUAL, K_RESID, K_BWD}
    assert {p[3] for p in plans} == {0, 1, 2, 3}
    for tile in (64, 12864, 128):
        full = {c.plan[2] for c in CASES if c.plan[1] == tile and c.why.startswith("full") and not c.off}
        ragged = {c.plan[2] for c in CASES if c.plan[1] == tile and c.why.startswith("ragged")}
        assert full >= {GEN, STORE, K_DUAL, K_RESID, K_BWD}, (tile, full)
        assert ragged == {GEN, STORE}, (tile, ragged)
        # every epilogue family through the predicated rows of this tile class
        acts = {EPIS[c.epi].get("act", A_NONE) for c in CASES if c.plan[1] == tile and c.why.startswith("ragged")}
        assert acts >= {A_NONE, A_TANH} and acts & {A_DUAL, A_DUAL_D, A_DUAL_DK} and acts & {A_BWD, A_MUL_AUX}
        # a partial column group (nv < 4, vec_ok false), the per-element dropout hash of an odd
        # m * N + n, and column-sum rows that end inside a thread's four columns
        here = [c for c in CASES if c.plan[1] == tile]
        assert any(c.NO % 4 for c in here), tile
        assert any(c.NO % 2 and "drop" in EPIS[c.epi] for c in here), tile
        assert any(c.NO % 4 and "colsum" in EPIS[c.epi] for c in here), tile
        assert any(c.NO % 2 and "drop" in EPIS[c.epi] and "colsum" in EPIS[c.epi] for c in here), tile
    # the 64-row halves of a 128-row tile: the last tile's second half partly empty, empty,
    # and (the weight gradient's forced 128x128 tile) a whole problem of 64 < rows < 128
    for tile in (12864, 128):
        assert any(64 < c.M % 128 < 128 for c in CASES if c.plan[1] == tile), tile
    assert any(0 < c.M % 128 <= 64 for c in CASES if c.plan[1] == 12864)
    assert any(64 < n < 128 for n in WG_NS) and any(n < 64 for n in WG_NS)
    assert len({c.id for c in CASES}) == len(CASES)


@pytest.mark.parametrize("act", [A_DUAL, A_DUAL_D, A_DUAL_DK, A_GELU])
def test_colsum_with_gelu_dual_is_rejected(hv, act):
    """The GELU_DUAL family stops before the column sums (include/hvit.h): asking for both
    is an argument error on full and ragged shapes alike.  Asked through hvit_gemm_plan, which
    runs hvit_linear_fwd's own checks (check_epi among them) and can launch nothing."""
    L = hv._lib
    e = L.Epilogue()
    e.act, e.out2, e.out2_dt, e.colsum = act, 0x2000, BF16, 0x3000
    for M in (128, 100):
        p = L.GemmPlan()
        with pytest.raises(RuntimeError, match="colsum"):
            L.call("hvit_gemm_plan", FWD, BF16, M, 128, 64, None, 0x6000, BF16, e, 0, ctypes.byref(p))


# --------------------------------------------------------------- reference ---
def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v * 2.0 ** -0.5))


def gelu_grad64(v):
    return 0.5 * (1.0 + torch.erf(v * 2.0 ** -0.5)) + v * torch.exp(-0.5 * v * v) * (2.0 * torch.pi) ** -0.5


def epilogue_ref(acc, act, bias=None, rowadd=None, keep=None, aux=None, resid=None, rowscale=None):
    """include/hvit.h's epilogue in float64.  keep: the dropout multiplier (mask / (1 - p)) or
    None.  Returns (y, out2, column sums); the GELU_DUAL family has no column sums, ACT_GELU no out2."""
    M = acc.shape[0]
    rows = torch.arange(M, device=acc.device)
    v = acc.clone()
    if bias is not None:
        v = v + bias.double()
    if rowadd is not None:
        v = v + rowadd.double()[rows % rowadd.shape[0]]
    k = keep if keep is not None else torch.ones_like(v)
    if act in (A_DUAL, A_DUAL_D, A_DUAL_DK, A_GELU):
        g = gelu64(v) * k
        if act == A_GELU:
            return g, None, None
        d = gelu_grad64(v)
        return {A_DUAL: v, A_DUAL_D: d, A_DUAL_DK: d * k}[act], g, None
    if act == A_TANH:
        v = torch.tanh(v)
    v = v * k
    if act == A_BWD:
        v = v * gelu_grad64(aux.double())
    if act == A_MUL_AUX:
        v = v * aux.double()
    if resid is not None:
        rs = rowscale.double()[rows // RPS][:, None] if rowscale is not None else 1.0
        v = resid.double() + rs * v
    return v, None, v.sum(0)


# ------------------------------------------------------------ guard bands ---
class Guarded:
    """rows x cols of dtype inside a NaN buffer, a BAND_ROWS-row band on either side;
    off: the view starts one element past the 16-byte boundary."""

    def __init__(self, rows, cols, dtype, off=False, band_cols=None):
        self.band = BAND_ROWS * (band_cols or cols) + 8
        self.lo = self.band + (1 if off else 0)
        self.n = rows * cols
        self.buf = torch.full((self.lo + self.n + self.band,), NAN, device=DEV, dtype=dtype)
        self.t = self.buf[self.lo:self.lo + self.n].view(rows, cols)
        assert (self.t.data_ptr() % 16 != 0) == bool(off)
        self.bits = torch.int32 if dtype == torch.float32 else torch.int16
        self.sentinel = self.buf[:1].view(self.bits).clone()

    def refill(self):
        self.buf.fill_(NAN)

    def check(self, what):
        b = self.buf.view(self.bits)
        lo, hi = b[:self.lo], b[self.lo + self.n:]
        assert bool((lo == self.sentinel).all()) and bool((hi == self.sentinel).all()), \
            f"{what}: wrote outside its {self.t.shape[0]} x {self.t.shape[1]} output"
        bad = int((~torch.isfinite(self.t)).sum())
        assert bad == 0, f"{what}: {bad} of {self.n} elements not written"


def shifted(t):
    """t's values in storage that starts one element past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 != 0
    return v


def s():
    return torch.cuda.current_stream().cuda_stream


def check(out, ref, odt, acc, what):
    (check_f32 if odt == "f32" else check_bf16)(out, ref, acc=acc, what=what)


# ------------------------------------------------------------- fwd / dgrad ---
@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_linear_edges(hv, gemm_h_only, c):
    L = hv._lib
    torch.backends.cuda.matmul.allow_tf32 = False
    gen = torch.Generator(device=DEV).manual_seed(97)
    rnd = lambda *sh: torch.randn(*sh, device=DEV, generator=gen)  # noqa: E731
    spec, M, NO, KR = EPIS[c.epi], c.M, c.NO, c.KR
    act = spec.get("act", A_NONE)
    a = rnd(M, KR).to(tdt(c.dt))
    if c.entry == FWD:
        w = (rnd(NO, KR) * KR ** -0.5).to(tdt(c.dt))
        acc = a.double() @ w.double().t()
    else:
        w = (rnd(KR, NO) * KR ** -0.5).to(tdt(c.dt))
        acc = a.double() @ w.double()
    bias = rnd(NO) if "bias" in spec else None
    rowadd = rnd(RA_ROWS, NO) if "rowadd" in spec else None
    aux = None
    if "aux" in spec:
        aux = rnd(M, NO).to(tdt(c.dt))
        if c.off == "aux":
            aux = shifted(aux)
    resid = None
    if "resid" in spec:
        resid = shifted(rnd(M, NO)) if c.off == "resid" else rnd(M, NO)
    rowscale = None
    if "rowscale" in spec:
        rowscale = torch.rand((M + RPS - 1) // RPS, device=DEV, generator=gen) + 0.5
        rowscale[1::3] = 0.0  # dropped paths
    mask = keep = None
    if "drop" in spec:
        mask = torch.as_tensor(keep_mask(SEED, SITE, M * NO, P_DROP).reshape(M, NO), device=DEV)
        keep = mask.double() / (1.0 - P_DROP)
    ref_y, ref_o2, ref_cs = epilogue_ref(acc, act, bias, rowadd, keep, aux, resid, rowscale)

    y = Guarded(M, NO, tdt(c.odt), off=c.off == "y")
    out2 = Guarded(M, NO, tdt(c.odt), off=c.off == "out2") if "out2" in spec else None
    cs = Guarded((M + 63) // 64, NO, torch.float32) if "colsum" in spec else None
    ptrs = {"y": (y.t.data_ptr(), c.odt)}
    for name, t in (("out2", out2 and out2.t), ("aux", aux), ("resid", resid), ("rowscale", rowscale),
                    ("rowadd", rowadd), ("colsum", cs and cs.t), ("bias", bias)):
        if t is not None:
            ptrs[name] = (t.data_ptr(), "f32" if t.dtype == torch.float32 else "bf16")
    # the plan, from the launcher's own decision code, before anything runs
    assert query(L, c, ptrs) == c.plan
    e = make_epi(L, c, ptrs)
    N, K = c.api_nk()
    acc_y = 1e-4 if c.epi in GELU_EPIS and act != A_DUAL else ACC  # (GELU_DUAL's y is the pre-activation)
    for knob in (0, -1):  # gemm.h's kernels, then the automatic choice
        gemm_h_only(knob)
        for g in (y, out2, cs):
            if g is not None:
                g.refill()
        what = f"{c.id} knob {knob}"
        if c.entry == FWD:
            L.call("hvit_linear_fwd", dtc(c.dt), a.data_ptr(), w.data_ptr(), L.ptr(bias), M, N, K, y.t.data_ptr(),
                   dtc(c.odt), e, s())
        else:
            L.call("hvit_linear_dgrad", dtc(c.dt), a.data_ptr(), w.data_ptr(), M, N, K, y.t.data_ptr(), dtc(c.odt),
                   e, s())
        torch.cuda.synchronize()
        y.check(what + " y")
        check(y.t, ref_y, c.odt, acc_y, what + " y")
        if out2 is not None:
            out2.check(what + " out2")
            check(out2.t, ref_o2, c.odt, 1e-4, what + " out2")
        if cs is not None:
            cs.check(what + " colsum rows")
            check_f32(cs.t.double().sum(0), ref_cs, acc=1e-4 if c.epi in GELU_EPIS else ACC, what=what + " colsum")
        if mask is not None and act == A_NONE and resid is None:
            assert torch.equal(y.t == 0, ~mask), what + ": the zeros are not the dropout mask's"
        if mask is not None and act in (A_DUAL, A_DUAL_D, A_DUAL_DK, A_GELU):
            # gelu(v) is zero only where v is: the dropped elements are exactly zero
            o = out2.t if out2 is not None else y.t
            assert bool((o[~mask] == 0).all()), what + ": a dropped element is not zero"


# ------------------------------------------------------------------- wgrad ---
@pytest.mark.parametrize("N,dt,db_form,with_ws,ek,splits", WGRAD_CASES)
def test_wgrad_plans(hv, gemm_h_only, N, dt, db_form, with_ws, ek, splits):
    """(no GPU) the ragged weight gradient's plan: gemm.h's 128x128 tile, split-K slabs with
    a workspace, a plain store without."""
    L = hv._lib
    M, K = WG_M, WG_K
    ws_n = L.lib().hvit_wgrad_workspace(M, N, K) if with_ws else 0
    assert not with_ws or ws_n >= 3 * (N * K + N)
    dw = 0x100000
    db = {"none": None, "fused": dw + 4 * N * K, "separate": 0x200000}[db_form]
    p = L.GemmPlan()
    L.call("hvit_gemm_plan", WGRAD, dtc(dt), M, N, K, db, dw, F32, None, ws_n, ctypes.byref(p))
    assert p.astuple() == (0, 128, ek, 0) and p.splits == splits


@pytest.mark.gpu
@pytest.mark.parametrize("N,dt,db_form,with_ws,ek,splits", WGRAD_CASES)
def test_linear_wgrad_edges(hv, gemm_h_only, N, dt, db_form, with_ws, ek, splits):
    L = hv._lib
    M, K = WG_M, WG_K
    gen = torch.Generator(device=DEV).manual_seed(98)
    dy = torch.randn(M, N, device=DEV, generator=gen).to(tdt(dt))
    x = torch.randn(M, K, device=DEV, generator=gen).to(tdt(dt))
    ref_dw = dy.double().t() @ x.double()
    ref_db = dy.double().sum(0)
    ws_n = L.lib().hvit_wgrad_workspace(M, N, K) if with_ws else 0
    ws = torch.full((max(ws_n, 1),), NAN, device=DEV) if with_ws else None
    if db_form == "fused":  # db == dw + N * K: one output of N rows of K and one of N
        g = Guarded(N * K + N, 1, torch.float32, band_cols=K)
        dw, db, dbg = g.t.view(-1)[:N * K].view(N, K), g.t.view(-1)[N * K:], None
    else:
        g = Guarded(N, K, torch.float32)
        dw = g.t
        dbg = Guarded(1, N, torch.float32) if db_form == "separate" else None
        db = dbg.t.view(-1) if dbg is not None else None
    p = L.GemmPlan()
    L.call("hvit_gemm_plan", WGRAD, dtc(dt), M, N, K, L.ptr(db), dw.data_ptr(), F32, None, ws_n, ctypes.byref(p))
    assert p.astuple() == (0, 128, ek, 0) and p.splits == splits
    for knob in (0, -1):
        gemm_h_only(knob)
        g.refill()
        if dbg is not None:
            dbg.refill()
        what = f"wgrad N {N} {dt} db {db_form} ws {with_ws} knob {knob}"
        L.call("hvit_linear_wgrad", dtc(dt), dy.data_ptr(), x.data_ptr(), M, N, K, dw.data_ptr(), L.ptr(db),
               L.ptr(ws), ws_n, s())
        torch.cuda.synchronize()
        g.check(what)
        check_f32(dw, ref_dw, acc=1e-4, what=what + " dw")
        if db is not None:
            if dbg is not None:
                dbg.check(what + " db")
            check_f32(db, ref_db, acc=1e-4, what=what + " db")
