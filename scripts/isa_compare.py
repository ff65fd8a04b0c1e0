"""Compare the decode-projection kernels of two gfx950 assembly listings of vl2_abi.hip (hipcc --save-temps: the *-gfx950.s file), kernel by
kernel: VGPRs, SGPRs, LDS, scratch, occupancy and whether the instruction text is identical once symbol names, local labels and kernarg
offsets are normalised.  Prints a markdown table.

    python scripts/isa_compare.py PARENT.s CHANGE.s > table.md
"""
import re
import subprocess
import sys

FAMILIES = ("gemm_skinny_kernel", "gemm_skinny_fp8_kernel", "gemm_skinny_mxfp4_kernel", "gemv_fp8_kernel", "gemv_mr_fp8_kernel", "gemv_mxfp4_kernel",
            "gemv_mr_mxfp4_kernel", "gemv_bf16_kernel", "gemv_mr_bf16_kernel", "gemv_xfirst_bf16_kernel", "skinny_reduce_kernel", "moe_gemv_gu_kernel")
KEYS = (("vgpr", "TotalNumVgprs"), ("sgpr", "TotalNumSgprs"), ("lds", "LDSByteSize"), ("scratch", "ScratchSize"), ("occ", "Occupancy"))


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def parse(path):
    """kernel symbol -> its instruction text and the figures of the "; Kernel info:" block that follows it"""
    txt = open(path).read()
    kernels = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:.*?^; Kernel info:\n(.*?)^; COMPUTE_PGM", txt, re.M | re.S):
        k = {"body": m.group(2)}
        for key, d in KEYS:
            k[key] = int(re.search(r"^; " + d + r"\s*:\s*(\d+)", m.group(3), re.M).group(1))
        kernels[m.group(1)] = k
    return kernels


def normal(body):
    lines = []
    for ln in body.split("\n"):
        ln = ln.split(";")[0].rstrip()
        if not ln.strip() or ln.strip().startswith("."):
            if not re.match(r"^\.LBB", ln.strip()):
                continue
        ln = re.sub(r"\.LBB\d+_", ".LBB_", ln)
        ln = re.sub(r"_Z\w+", "SYM", ln)
        lines.append(ln)
    return lines


def main(parent, change):
    P, C = parse(parent), parse(change)
    dm = demangle(sorted(set(P) | set(C)))
    strip = lambda s: re.sub(r"\(.*\)$", "", s.replace("void ", ""))          # the argument struct's name may differ: compare by kernel<...>
    pn = {strip(dm[k]): k for k in P}
    cn = {strip(dm[k]): k for k in C}
    rows = []
    for name in sorted(set(pn) | set(cn)):
        if not name.startswith(FAMILIES) or name.split("<")[0] not in FAMILIES:
            continue
        p, c = P.get(pn.get(name)), C.get(cn.get(name))
        if p is None or c is None:
            rows.append((name, "only in " + ("change" if p is None else "parent"), "", "", "", "", ""))
            continue
        a, b = normal(p["body"]), normal(c["body"])
        ops = lambda ls: sorted(x.split()[0] for x in ls if not x.startswith(".") and not x.split()[0].startswith(("s_cbranch", "s_branch")))
        if a == b:
            verdict = "identical"
        elif sorted(x for x in a if "branch" not in x and not x.startswith(".")) == sorted(x for x in b if "branch" not in x and not x.startswith(".")):
            verdict = "same instructions, other block order"
        elif ops(a) == ops(b):
            verdict = "same opcode counts, other registers / order"
        else:
            oa, ob = ops(a), ops(b)
            delta = sum(abs(oa.count(o) - ob.count(o)) for o in set(oa) | set(ob))
            verdict = f"differs ({len(oa)} -> {len(ob)} instructions, {delta} opcode count changes)"
        f = lambda k: f"{p.get(k)}" if p.get(k) == c.get(k) else f"{p.get(k)} -> {c.get(k)}"
        rows.append((name, verdict, f("vgpr"), f("sgpr"), f("lds"), f("scratch"), f("occ")))
    print("| kernel | ISA text | VGPRs | SGPRs | static LDS | scratch | occupancy |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        print("| `" + r[0] + "` | " + " | ".join(r[1:]) + " |")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
