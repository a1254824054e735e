#!/usr/bin/env python3
"""Compare named kernels between two gfx950 assembly files (hipcc --save-temps) and record their registers.

  python scripts/asm_kernel_diff.py PARENT.s NEW.s --same K1,K2 [--new-kernels K3,K4] [--csv OUT.csv]
                                     [--opcodes] [--loop]

A kernel is matched by a substring of its (mangled) symbol.  Its instruction stream is every line between the symbol's
label and its s_endpgm block, comments stripped; basic-block labels are kept (they are numbered per function, so an
unchanged function keeps them).  --same kernels must have the same stream in both files (exit 1 otherwise, with the
unified diff); --new-kernels exist only in NEW.  The csv holds VGPR / AGPR / SGPR / private-segment / spill figures read
from each kernel's .amdhsa_ descriptor and its resource-usage comments.

--opcodes compares the sequences of mnemonics only (operands, so register numbers, and labels left out): what a refactor
that only moves code between functions may change without changing the schedule.  A difference is reported and
recorded, not an error.  --loop adds the main loop's counts to the csv: the span from the label that the first backward
branch after the last MFMA targets, to that branch (MFMAs, s_barrier, buffer_load ... lds, ds_read_b128,
ds_read_b64_tr_b16, s_waitcnt vmcnt sites, s_load, instructions).
"""
import argparse
import difflib
import re
import sys


def kernels(path):
    """symbol -> {"stream": [instruction lines], "meta": {...}} for every .amdhsa_kernel of the file"""
    text = open(path).read().splitlines()
    out = {}
    syms = [m.group(1) for ln in text if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln))]
    for sym in syms:
        start = next(i for i, ln in enumerate(text) if ln.startswith(sym + ":"))
        end = next(i for i in range(start, len(text)) if text[i].startswith(".Lfunc_end"))
        stream = []
        for ln in text[start + 1:end]:
            ln = ln.split(";")[0].rstrip()
            if ln.strip() and not ln.strip().startswith((".p2align", ".section", ".loc", ".cfi", ".file")):
                stream.append(ln.strip())
        meta = {}
        d0 = next(i for i, ln in enumerate(text) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(sym) + r"$", ln))
        for ln in text[d0:]:
            if ".end_amdhsa_kernel" in ln:
                break
            m = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", ln)
            if m:
                meta[m.group(1)] = m.group(2)
        for ln in text[end:end + 60]:  # the "; Kernel info:" comments after the function
            m = re.match(r";\s*(TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize)\s*:\s*(\d+)", ln)
            if m:
                meta.setdefault(m.group(1), m.group(2))
        y0 = next(i for i, ln in enumerate(text) if re.match(r"\s*\.name:\s+" + re.escape(sym) + r"$", ln))
        for ln in text[y0 + 1:]:  # the metadata note: keys of one kernel in alphabetical order
            m = re.match(r"\s*\.(sgpr_spill_count|vgpr_spill_count|name):\s+(\S+)", ln)
            if m and m.group(1) == "name":
                break
            if m:
                meta[m.group(1)] = m.group(2)
        out[sym] = {"stream": stream, "meta": meta}
    return out


def pick(ks, name):
    hits = [s for s in ks if name in s]
    # "attn_fwd_v6_kernel" must not match "attn_fwd_v6_sparse_kernel": the mangled form is <len><name>
    exact = [s for s in hits if f"{len(name)}{name}" in s]
    hits = exact or hits
    if len(hits) != 1:
        raise SystemExit(f"{name}: {len(hits)} kernels match ({hits})")
    return hits[0]


LOOP_COLS = [("loop_mfma", r"v_mfma"), ("loop_barrier", r"s_barrier"), ("loop_lds_dma", r"buffer_load_\S+ .* lds"),
             ("loop_ds_read_b128", r"ds_read_b128"), ("loop_ds_read_tr", r"ds_read_b64_tr_b16"),
             ("loop_vmcnt", r"s_waitcnt .*vmcnt"), ("loop_s_load", r"s_load_"), ("loop_len", r"[^.]")]


def opcodes(stream):
    return [ln.split()[0] for ln in stream if not ln.endswith(":")]


def loop_counts(stream):
    """the LOOP_COLS counts over the main loop, "" each for a kernel without MFMAs or without such a loop"""
    labels = {ln[:-1]: i for i, ln in enumerate(stream) if ln.endswith(":")}
    mf = [i for i, ln in enumerate(stream) if ln.startswith("v_mfma")]
    for i in range(mf[-1] + 1 if mf else len(stream), len(stream)):
        m = re.match(r"s_c?branch\S*\s+(\S+)", stream[i])
        if m and labels.get(m.group(1), len(stream)) < mf[-1]:
            span = [ln for ln in stream[labels[m.group(1)]:i + 1] if not ln.endswith(":")]
            return [str(sum(1 for ln in span if re.match(rx, ln))) for _, rx in LOOP_COLS]
    return [""] * len(LOOP_COLS)


def row(label, k, same="", loop=False):
    m = k["meta"]
    g = lambda *names: next((m[n] for n in names if n in m), "")
    mfma = sum(1 for ln in k["stream"] if ln.startswith("v_mfma"))
    return ",".join([label, g("NumVgprs"), g("NumAgprs"), g("TotalNumSgprs"), g("next_free_vgpr"), g("accum_offset"),
                     g("ScratchSize", "private_segment_fixed_size"), g("vgpr_spill_count"),
                     g("sgpr_spill_count"), str(sum(1 for ln in k["stream"] if not ln.endswith(":"))),
                     str(mfma), same] + (loop_counts(k["stream"]) if loop else []))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--same", default="")
    ap.add_argument("--new-kernels", dest="newk", default="")
    ap.add_argument("--csv")
    ap.add_argument("--opcodes", action="store_true")
    ap.add_argument("--loop", action="store_true")
    a = ap.parse_args()
    kp, kn = kernels(a.parent), kernels(a.new)
    rows = ["kernel,vgpr,agpr,sgpr,next_free_vgpr,accum_offset,private_segment_bytes,vgpr_spills,sgpr_spills,"
            "instructions,mfma,same_stream_as_parent" + "".join("," + c for c, _ in LOOP_COLS if a.loop)]
    bad = 0
    for name in filter(None, a.same.split(",")):
        p, n = kp[pick(kp, name)], kn[pick(kn, name)]
        ps, ns = (opcodes(p["stream"]), opcodes(n["stream"])) if a.opcodes else (p["stream"], n["stream"])
        same = ps == ns
        print(f"{name}: {len(n['stream'])} lines, {'identical' if same else 'DIFFERENT'}")
        if not same:
            bad += not a.opcodes
            d = list(difflib.unified_diff(ps, ns, "parent", "new", lineterm=""))
            print(f"  {sum(1 for ln in d if ln.startswith('@@'))} hunks, -{sum(1 for ln in d if ln[:1] == '-') - 1} "
                  f"+{sum(1 for ln in d if ln[:1] == '+') - 1} lines")
            sys.stdout.writelines(ln + "\n" for ln in d[:80])
        what = "opcodes " if a.opcodes else ""
        rows.append(row(name + " (parent commit)", p, loop=a.loop))
        rows.append(row(name, n, what + ("identical" if same else "different"), loop=a.loop))
    for name in filter(None, a.newk.split(",")):
        rows.append(row(name, kn[pick(kn, name)], loop=a.loop))
    if a.csv:
        with open(a.csv, "w") as f:
            f.write("\n".join(rows) + "\n")
    print("\n".join(rows))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
