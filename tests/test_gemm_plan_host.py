"""The launch plan of vl2_gemm (csrc/gemm_plan.h) on the CPU, against tests/golden/gemm_plan_table.txt: the launches that the launcher which the
plan replaced made for these calls (recorded from its host side, product and lab builds) -- kernel form, tile, rows, tile counts, grid, template
switches, workspace wiring and whether a row_norm_finalize launch follows.  Every kernel of the family produces the same bits, so the GPU tests
cannot see a slip in this choice; this table is what pins it."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "gemm_plan_table.txt")
IN_KEYS = "M N K act sw f32 g remap fp8 res so norm rn rno tctr ws wsb v splitk pers nomix nofill weave weave4 noweave4 mfma16 cus lab".split()

SHIM = r'''
#include "gemm_plan.h"
#include <stdio.h>
// i: the table's input columns in order; out: "<finalize> | launch ; launch" in the table's words
extern "C" int plan(const long long* i, char* out, int cap) {
    GemmPlanIn a{};
    a.M = (int)i[0]; a.N = (int)i[1]; a.K = (int)i[2]; a.act = i[3]; a.swiglu = i[4]; a.f32 = i[5]; a.gather = i[6]; a.remap = i[7]; a.fp8 = i[8];
    a.res = i[9]; a.stats_out = i[10]; a.norm = i[11]; a.row_norm = i[12]; a.row_norm_out = i[13]; a.tile_ctr = i[14]; a.ws = i[15]; a.ws_bytes = i[16];
    a.variant = (int)i[17]; a.splitk = i[18]; a.persist = i[19]; a.no_mix = i[20]; a.no_fill = i[21]; a.weave = i[22]; a.weave4 = i[23]; a.no_weave4 = i[24];
    a.cus = (int)i[26]; a.lab = i[27];
    a.mfma16 = want_mfma16(a, i[25] != 0);              // as vl2_gemm decides it, from the VL2_GEMM_MFMA16 bit
    const GemmPlan p = gemm_plan(a);
    bool fin = false;
    for (int k = 0; k < p.n; ++k) fin = fin || p.l[k].needs_finalize;
    int n = snprintf(out, cap, "%d |", (int)fin);
    for (int k = 0; k < p.n; ++k) {
        const GemmLaunch& l = p.l[k];
        n += snprintf(out + n, cap - n, "%s %s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", k ? " ;" : "", kGemmFormName[l.form], l.tile_h, l.tile_w, l.m0, l.rows,
                      l.tiles_m, l.tiles_n, l.grid_x, l.grid_y, (int)l.tr, (int)l.woven, l.mode, (int)l.acc2, l.split, l.dyn, l.tile_group, (int)l.ws_wired, l.tail_rows,
                      l.tail_tiles_m, l.tail_tiles_n, l.tail_tile_group);
    }
    return p.n;
}
'''

# the forms the automatic choice (variant 0) can reach in the product build: each must stay in the table
PRODUCT_AUTO_FORMS = {"GF_128", "GF_128_SPLITK", "GF_64", "GF_L8", "GF_128x256", "GF_G4_256", "GF_G4_192", "GF_GEMM6", "GF_GEMM7", "GF_GEMM9", "GF_MIX", "GF_MIX16",
                      "GF_L8_16", "GF_REMAP", "GF_FP8_128x256", "GF_FP8_256", "GF_FP8_192"}


def _rows():
    rows = []
    for line in open(TABLE):
        if line.startswith("#") or not line.strip():
            continue
        ins, fin, launches = (p.strip() for p in line.split("|"))
        rows.append(([int(x) for x in ins.split()], fin + " | " + " ; ".join(l.strip() for l in launches.split(";"))))
    return rows


@pytest.fixture(scope="module")
def plan_lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("gemm_plan")
    src, so = d / "plan.cpp", d / "plan.so"
    src.write_text(SHIM)
    cxx = "/opt/rocm/lib/llvm/bin/clang++"
    subprocess.run([cxx if os.path.exists(cxx) else "c++", "-O1", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "videollama2_amd", "csrc"),
                    str(src), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.plan.argtypes = [ctypes.POINTER(ctypes.c_longlong), ctypes.c_char_p, ctypes.c_int]
    return lib


def test_gemm_plan_gives_the_recorded_launches(plan_lib):
    rows = _rows()
    assert 300 <= len(rows) <= 500
    out = ctypes.create_string_buffer(1024)
    bad = []
    for ins, want in rows:
        assert len(ins) == len(IN_KEYS)
        n = plan_lib.plan((ctypes.c_longlong * len(ins))(*ins), out, len(out))
        got = out.value.decode()
        if got != want or n != want.count(";") + 1:
            bad.append(f"{dict(zip(IN_KEYS, ins))}\n   plan   {got}\n   table  {want}")
    assert not bad, f"{len(bad)} of {len(rows)} plans differ from the recorded launches:\n" + "\n".join(bad[:8])


def test_table_reaches_every_form_of_the_automatic_choice():
    """A later edit cannot hollow the table out: every kernel form that variant 0 reaches in the product build is there, on variant 0 and lab = 0;
    so are a two-launch row split, a plan that leaves row_norm_out to the finalize launch, the lab-only forms, a row for every input column that a
    branch reads and one for every accepted variant."""
    rows = _rows()
    v, lab = IN_KEYS.index("v"), IN_KEYS.index("lab")
    forms = lambda want: {l.split()[0] for l in want.split("|")[1].split(";")}
    auto = set().union(*(forms(want) for ins, want in rows if ins[v] == 0 and ins[lab] == 0))
    assert auto >= PRODUCT_AUTO_FORMS, sorted(PRODUCT_AUTO_FORMS - auto)
    assert any(ins[v] == 0 and ins[lab] == 0 and ";" in want for ins, want in rows), "no two-launch row split"
    assert any(ins[v] == 0 and ins[lab] == 0 and want.startswith("1 |") for ins, want in rows), "no plan without a producer-side finalize"
    every = set().union(*(forms(want) for _, want in rows))
    assert every >= PRODUCT_AUTO_FORMS | {"GF_128_STREAMK", "GF_G4_160", "GF_GEMM8", "GF_GEMM7_16"}, sorted(every)
    # the branches that read one input column, each on the automatic choice of the product build ...
    col = {k: i for i, k in enumerate(IN_KEYS)}
    auto_rows = [ins for ins, _ in rows if ins[v] == 0 and ins[lab] == 0]
    for name, pred in (("activation, K < 2048", lambda r: r[col["act"]] and r[col["K"]] < 2048), ("activation, K >= 2048", lambda r: r[col["act"]] and r[col["K"]] >= 2048),
                       ("gathered", lambda r: r[col["g"]]), ("norm with row_norm + PERSISTENT", lambda r: r[col["norm"]] and r[col["rn"]] and r[col["pers"]]),
                       ("norm without row_norm + PERSISTENT", lambda r: r[col["norm"]] and not r[col["rn"]] and r[col["pers"]]), ("NO_FILL", lambda r: r[col["nofill"]]),
                       ("NO_MIX", lambda r: r[col["nomix"]]), ("SPLITK with a workspace", lambda r: r[col["splitk"]] and r[col["ws"]]), ("MFMA16", lambda r: r[col["mfma16"]]),
                       ("residual", lambda r: r[col["res"]]), ("SwiGLU", lambda r: r[col["sw"]]), ("fp32 out", lambda r: r[col["f32"]])):
        assert any(pred(r) for r in auto_rows), f"no row for: {name}"
    # ... every variant vl2_gemm accepts (the lab forms on lab = 1; 24 = the re-planned automatic choice), and the fp8 form's forced variants
    PRODUCT_VARIANTS = {0, 1, 4, 8, 12, 16, 24, 26, 32, 60, 61, 70, 71, 80, 81, 192, 224, 256}
    LAB_VARIANTS = {2, 5, 9, 10, 17, 18, 19, 20, 21, 22, 23, 25, 27, 28, 29, 62, 193, 225}
    assert {ins[v] for ins, _ in rows if ins[lab] == 0 and not ins[col["fp8"]]} == PRODUCT_VARIANTS
    assert {ins[v] for ins, _ in rows if ins[lab] == 1} >= LAB_VARIANTS
    assert {ins[v] for ins, _ in rows if ins[col["fp8"]]} == {0, 4, 8, 12}
    assert any(ins[v] == 16 and ins[col["sw"]] and "GF_MIX16" in want for ins, want in rows), "variant 16 on a SwiGLU row split (MODE 0)"
    assert any(ins[v] in (224, 192) and not ins[col["mfma16"]] for ins, _ in rows) and any(ins[v] in (224, 192) and ins[col["mfma16"]] for ins, _ in rows)
