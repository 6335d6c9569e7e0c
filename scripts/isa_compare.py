"""Compare the gfx950 device code of two builds, function by function.

    python scripts/isa_compare.py [--summary] --parent A.s [B.s ...] --new C.s [D.s ...]

The inputs are hipcc's assembly listings (the Makefile's HIPFLAGS plus
--cuda-device-only -S).  Per function (kernels, and device functions that were
not inlined) it prints the metadata's VGPR / SGPR / AGPR counts, scratch,
static LDS and kernarg bytes, the SGPR / VGPR spill counts, the number of MFMA,
VALU (v_* other than v_mfma*) and s_nop instructions, the number of
instruction / label / directive lines and their SHA-1 after normalising (comments stripped; block,
function-end and jump-table labels numbered relative to the function), then a
unified diff of every function whose stream, .amdhsa_kernel descriptor or
metadata differ (--summary: the table only).  It hashes and compares; it runs
nothing.
"""
import argparse
import difflib
import hashlib
import re
import subprocess

LABEL = re.compile(r"\.L(BB|JTI|func_begin|func_end|tmp)\d+(_?)")
META = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("agpr", ".agpr_count"),
        ("scratch", ".private_segment_fixed_size"), ("lds", ".group_segment_fixed_size"),
        ("kernarg", ".kernarg_segment_size"), ("sspill", ".sgpr_spill_count"), ("vspill", ".vgpr_spill_count"))


def norm(line):
    line = line.split(";")[0].rstrip()
    return LABEL.sub(lambda m: ".L" + m.group(1) + m.group(2), line)


def parse(paths):
    """{symbol: {"body": [...], "desc": [...], "meta": {...}}} over the listings."""
    funcs = {}
    for path in paths:
        lines = open(path).read().splitlines()
        types = {m.group(1) for m in (re.match(r"\s*\.type\s+(\w+),@function", ln) for ln in lines) if m}
        cur = desc = None
        meta = None
        in_meta = False
        for ln in lines:
            s = norm(ln)
            if not s.strip():
                continue
            m = re.match(r"(\w+):$", s)
            if m and m.group(1) in types:
                cur = funcs.setdefault(m.group(1), {"body": [], "desc": [], "meta": {}})["body"]
                continue
            if cur is not None:
                if s.startswith(".Lfunc_end"):
                    cur = None
                else:
                    cur.append(s)
                continue
            m = re.match(r"\s*\.amdhsa_kernel\s+(\w+)", s)
            if m:
                desc = funcs.setdefault(m.group(1), {"body": [], "desc": [], "meta": {}})["desc"]
            elif s.strip() == ".end_amdhsa_kernel":
                desc = None
            elif desc is not None:
                desc.append(s.strip())
            elif s.strip() == "amdhsa.kernels:":
                in_meta = True
            elif in_meta and re.match(r"  - \.", s):  # a kernel's entry; its fields follow at this indent
                meta = {}
                k, _, v = s[4:].partition(":")
                meta[k.strip()] = v.strip()
            elif in_meta and meta is not None and re.match(r"    \.\w+:", s):
                k, _, v = s.strip().partition(":")
                meta[k] = v.strip()
                if k == ".name" and meta[k] in funcs:
                    funcs[meta[k]]["meta"] = meta
            elif in_meta and not s.startswith(" "):
                in_meta = False
    return funcs


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    short = {}
    for n, d in zip(names, out):
        d = d.replace("psvo::(anonymous namespace)::", "").replace("psvo::", "")
        short[n] = d.split("(")[0].replace("void ", "")
    return short


def describe(f):
    meta = " ".join(f"{k} {f['meta'].get(key, '?')}" for k, key in META)
    sha = hashlib.sha1("\n".join(f["body"]).encode()).hexdigest()[:12]
    ops = [ln.split()[0] for ln in f["body"] if ln.strip()]
    mfma = sum(o.startswith("v_mfma") for o in ops)
    valu = sum(o.startswith("v_") for o in ops) - mfma
    nops = sum(o == "s_nop" for o in ops)
    return f"{meta}  mfma {mfma} valu {valu} s_nop {nops}  insn-lines {len(f['body'])} sha1 {sha}"


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--parent", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--summary", action="store_true", help="the per-function table only, no diffs")
    a = ap.parse_args()
    P, N = parse(a.parent), parse(a.new)
    names = sorted(set(P) | set(N))
    short = demangle(names)
    wide = max(len(short[n]) for n in names)
    diffs = []
    for n in sorted(names, key=lambda n: short[n]):
        p, q = P.get(n), N.get(n)
        if p is None or q is None:
            verdict = "ONLY IN " + ("new" if p is None else "parent")
        else:
            keys = [key for _, key in META]
            same_meta = [p["meta"].get(k) for k in keys] == [q["meta"].get(k) for k in keys]
            if p["body"] == q["body"] and p["desc"] == q["desc"] and same_meta:
                verdict = "identical"
            else:
                d = list(difflib.unified_diff(p["body"] + p["desc"], q["body"] + q["desc"], "parent", "new", n=0,
                                              lineterm=""))
                changed = sum(1 for ln in d if ln[:1] in "+-" and ln[:3] not in ("+++", "---"))
                verdict = f"DIFFERS ({changed} lines{'' if same_meta else ', metadata'})"
                diffs.append((short[n], d))
        print(f"{short[n]:<{wide}} | parent: {describe(p) if p else '-'} | new:    {describe(q) if q else '-'} | {verdict}")
    print()
    print(f"{len(P)} parent functions, {len(N)} new, {len(diffs)} differing, "
          f"{sum(1 for n in names if n not in P or n not in N)} unmatched")
    for name, d in ([] if a.summary else diffs):
        print(f"\n{name}:")
        for ln in d[2:]:
            print("  " + ln)


if __name__ == "__main__":
    main()
