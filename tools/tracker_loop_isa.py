#!/usr/bin/env python3
"""What the compiler made of the dense tracker's sample loop (scavislam_amd/csrc/dense.hip, track_pass).

Has csrc/Makefile write the gfx950 assembly of dense.hip (build/dense.s: the unit's own flags, device only), finds the loop over the
samples in every function that inlines track_pass (the tracker kernels) and prints, per loop: instructions per trip by class,
the function's VGPRs / scratch / occupancy, the order in which the trip issues its memory operations and waits for them, and two verdicts:

    do all tap loads of a sample (the four rows of its 4 x 4 neighbourhood in the u8 image) go out before the first wait that covers one of them?

    does any vmcnt wait between the trip's first memory request (the deferred term store, the prefetch of the next sample's cloud point and
    previous-frame byte) and its first tap load force requests of THIS trip to complete?  vmcnt(N) leaves at most the N youngest requests open, loads and
    stores in one queue: behind k requests of the trip it makes k - N of them complete before the taps are even issued -- the prefetch is then no
    prefetch, and a trip pays two memory round trips one after the other (profiles/tracker_prefetch.md).

It also reports the function's LDS and, per loop, the vector-ALU instructions per processed sample (f64, f32, integer, quarter-rate, moves / selects; one
f64 reciprocal -- one projection -- marks a sample).  The sweep runs two trips per iteration on alternating register sets (profiles/tracker_sweep.md): such a
loop is listed as one entry per trip, each held to both verdicts on its own, and its per-sample count is the loop's count over its samples.

A tracker whose taps are waited for row by row pays one memory round trip per row and sample; the compiler chose that once, silently, at the
128-register limit of the big-batch kernels (profiles/tracker_taps.md).  tests/test_tracker_isa_cpu.py holds the two hot instantiations to the verdict.

    python tools/tracker_loop_isa.py                 # the working tree
    python tools/tracker_loop_isa.py --rev HEAD~1    # another commit (git archive into the temporary directory)
    python tools/tracker_loop_isa.py --asm dense.s   # an assembly file made elsewhere
    python tools/tracker_loop_isa.py --json          # the same as one JSON document
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("scavislam_amd", "csrc")
HOT = ("dense_track_batch_kernel<true, true, 0>", "dense_track_batch_kernel<true, false, 1>")
QUARTER = ("v_mul_lo_u32", "v_mul_hi_u32", "v_mul_hi_i32", "v_mul_lo_i32", "v_mad_u64_u32", "v_mad_i64_i32")
CLASSES = ("f64", "f32", "integer", "quarter-rate", "moves/selects", "VMEM", "LDS", "scalar", "other")


def find_hipcc():
    cand = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return cand if cand and os.path.exists(cand) and os.access(cand, os.X_OK) else None


def compile_asm(src_root, hipcc):
    """build/dense.s by the Makefile's own rule: the Makefile alone knows the flags (a revision from before that rule cannot be analysed)."""
    csrc = os.path.join(src_root, CSRC)
    r = subprocess.run(["make", "-C", csrc, "HIPCC=" + hipcc, "build/dense.s"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if r.returncode != 0:
        raise RuntimeError("make build/dense.s failed:\n" + r.stderr[-4000:])
    return open(os.path.join(csrc, "build", "dense.s")).read()


def checkout_rev(rev, tmp):
    dst = os.path.join(tmp, "rev")
    os.makedirs(dst)
    ar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC, "include"], stdout=subprocess.PIPE, check=True)
    subprocess.run(["tar", "-x", "-C", dst], input=ar.stdout, check=True)
    return dst


def pretty_name(mangled):
    """dense_track_batch_kernel<true, false, 1> from the mangled name (the tracker's template arguments are bools and ints)."""
    m = re.search(r"\d+(dense_track_batch_kernel|dense_track_cpu_sem_kernel)I((?:Lb[01]E|Li\d+E)+)E", mangled)
    if not m:
        return None
    args = ["true" if a == "b1" else "false" if a == "b0" else a[1:] for a in re.findall(r"L(b[01]|i\d+)E", m.group(2))]
    name = "%s<%s>" % (m.group(1), ", ".join(args))
    if mangled.startswith("_ZZ"):
        name += " :: lambda"
    return name


def split_functions(text):
    """[(mangled name, body lines, {NumVgprs, ScratchSize, Occupancy, ...})] of an AMDGPU assembly file."""
    out, name, body = [], None, []
    lines = text.split("\n")
    i = 0
    while i < len(lines):
        ln = lines[i]
        m = re.match(r"^(_Z\w+):", ln)
        if m and name is None:
            name, body = m.group(1), []
        elif name is not None:
            body.append(ln)
            if ln.startswith(".Lfunc_end"):
                info = {}
                j = i + 1
                while j < len(lines) and not re.match(r"^(_Z\w+):", lines[j]) and j < i + 80:
                    mi = re.match(r"^; (\w+): (\d+)\s*(bytes/workgroup.*)?$", lines[j])      # ("; LDSByteSize: 17744 bytes/workgroup (compile time only)")
                    if mi:
                        info[mi.group(1)] = int(mi.group(2))
                    j += 1
                out.append((name, body, info))
                name = None
        i += 1
    return out


def instr_class(op):
    if op.startswith(("global_", "flat_", "scratch_", "buffer_")):
        return "VMEM"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith("s_"):
        return "scalar"
    if not op.startswith("v_"):
        return "other"
    if "f64" in op:
        return "f64"
    if "f32" in op or "f16" in op:
        return "f32"
    if op.startswith(QUARTER):
        return "quarter-rate"
    if op.startswith(("v_mov", "v_pk_mov", "v_cndmask", "v_readlane", "v_writelane", "v_readfirstlane", "v_accvgpr")):
        return "moves/selects"
    return "integer"


def parse_blocks(body):
    """Blocks in layout order: {label, header (label of the innermost loop the block lies in, or None), ins}."""
    blocks = [dict(label=None, header=None, ins=[])]
    for ln in body:
        m = re.match(r"^(\.LBB\d+_\d+):\s*(;.*)?$", ln) or re.match(r"^; %bb\.(\d+):\s*(;.*)?$", ln)
        if m:
            label = m.group(1) if m.group(1).startswith(".") else "bb." + m.group(1)
            h = re.search(r"in Loop: Header=(BB\d+_\d+)", m.group(2) or "")
            blocks.append(dict(label=label, header=".L" + h.group(1) if h else None, ins=[]))
            continue
        if ln.lstrip().startswith(";"):      # comments, among them ;;#ASMSTART / ;;#ASMEND: what an inline-asm statement holds is parsed like any other line
            continue
        s = ln.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        blocks[-1]["ins"].append(s)
    return blocks


def loops_of(body):
    """Innermost loops as instruction lists in trip order (from the loop's header round to the branch back to it)."""
    blocks = parse_blocks(body)
    # the label line of an innermost loop's header: "<label>: ; =>This Inner Loop Header: Depth=d", or the mark on a line of its own right after
    text_by_label = {}
    for ln_i, ln in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):(.*)$", ln)
        if m:
            k = ln_i + 1
            while k < len(body) and re.match(r"^\s+;", body[k]):      # (the comment lines that continue the label's own)
                k += 1
            text_by_label[m.group(1)] = m.group(2) + " " + " ".join(body[ln_i + 1:k])
    heads = [b["label"] for b in blocks if b["label"] and b["label"].startswith(".") and "This Inner Loop Header" in text_by_label.get(b["label"], "")]
    loops = []
    for h in heads:
        member = [k for k, b in enumerate(blocks) if b["label"] == h or b["header"] == h]
        if not member:
            continue
        start = next(k for k in member if blocks[k]["label"] == h)
        order = [k for k in member if k >= start] + [k for k in member if k < start]
        ins = [s for k in order for s in blocks[k]["ins"]]
        loops.append((h, ins))
    return loops


def vgprs_of(operand_text):
    regs = set()
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", operand_text):
        regs.update(range(int(a), int(b) + 1))
    regs.update(int(a) for a in re.findall(r"\bv(\d+)\b", operand_text))
    return regs


def is_tap_load(s):
    return re.match(r"^(global|flat)_load_dword\s", s) is not None


def is_vm_op(s):
    return s.startswith(("global_", "flat_", "buffer_", "scratch_")) and not s.startswith("global_wb") and not s.startswith("buffer_wbl2") and not s.startswith("buffer_inv")


def vmcnt_of(s):
    if not s.startswith("s_waitcnt"):
        return None
    m = re.search(r"vmcnt\((\d+)\)", s)
    if m:
        return int(m.group(1))
    m = re.match(r"^s_waitcnt\s+(0x[0-9a-fA-F]+|\d+)\s*$", s)      # a raw immediate: gfx9 vmcnt = bits 3:0 and 15:14
    if m:
        v = int(m.group(1), 0)
        return (v & 0xf) | (((v >> 14) & 0x3) << 4)
    return None


def analyse_loop(ins):
    counts = dict.fromkeys(CLASSES, 0)
    for s in ins:
        counts[instr_class(s.split()[0])] += 1
    mem_order = []
    for s in ins:
        if is_vm_op(s):
            mem_order.append(s.split()[0] + (" [tap]" if is_tap_load(s) else ""))
        elif vmcnt_of(s) is not None:
            mem_order.append("s_waitcnt vmcnt(%d)" % vmcnt_of(s))
    taps = [k for k, s in enumerate(ins) if is_tap_load(s)]
    res = dict(instructions=len(ins), classes=counts, memory_order=mem_order, tap_loads=len(taps), scratch_in_loop=sum(1 for s in ins if s.startswith("scratch_")),
               f64_fma=sum(1 for s in ins if re.match(r"^v_(fma|fmac)_f64", s)))
    if not taps:
        res.update(verdict=None, first_wait=None, taps_before_wait=0, dest_untouched=None, prefetch_waits=[], prefetch_forced=0, prefetch_verdict=None)
        return res
    # waits between the trip's first memory request and its first tap load: how many of the trip's own requests each forces to complete
    first_mem = next(k for k, s in enumerate(ins) if is_vm_op(s))
    waits = []
    for p in range(first_mem + 1, taps[0]):
        n = vmcnt_of(ins[p])
        if n is not None:
            issued = sum(1 for q in range(first_mem, p) if is_vm_op(ins[q]))
            waits.append(dict(wait="vmcnt(%d)" % n, issued=issued, forced=max(0, issued - n)))
    forced = max([w["forced"] for w in waits] or [0])
    res.update(prefetch_waits=waits, prefetch_forced=forced, prefetch_verdict=forced == 0)
    # the first wait behind the first tap load that covers one of the tap loads: vmcnt(N) leaves at most the N youngest requests open
    first_wait, covered_at = None, None
    for p in range(taps[0] + 1, len(ins)):
        n = vmcnt_of(ins[p])
        if n is None:
            continue
        for t in taps:
            if t < p and sum(1 for q in range(t + 1, p) if is_vm_op(ins[q])) >= n:
                first_wait, covered_at = p, n
                break
        if first_wait is not None:
            break
    before = sum(1 for t in taps if first_wait is None or t < first_wait)
    # between a tap load and that wait nothing may read or write the load's destination (the compiler does not track loads issued by inline assembly)
    untouched = True
    if first_wait is not None:
        for t in taps:
            if t > first_wait:
                continue
            dst = vgprs_of(ins[t].split(None, 1)[1].split(",")[0])
            for q in range(t + 1, first_wait):
                ops = ins[q].split(None, 1)
                if len(ops) > 1 and dst & vgprs_of(ops[1]):
                    untouched = False
    res.update(verdict=bool(first_wait is not None and before == len(taps)), first_wait="vmcnt(%d)" % covered_at if first_wait is not None else None,
               taps_before_wait=before, between_issue_and_wait=(first_wait - taps[-1] - 1) if first_wait is not None and before == len(taps) else 0,
               dest_untouched=untouched)
    return res


VALU_CLASSES = ("f64", "f32", "integer", "quarter-rate", "moves/selects")


def split_trips(ins):
    """The trips of a loop that handles several samples per iteration (track_pass runs two, on alternating register sets), in order.  A trip ends with the wait that
    covers its four tap loads plus what follows up to the next memory request; a loop of one sample, or of an f32 source (no tap loads), is one trip."""
    taps = [k for k, s in enumerate(ins) if is_tap_load(s)]
    if len(taps) <= 4 or len(taps) % 4:
        return [ins]
    cuts = [0]
    for g in range(4, len(taps), 4):
        k = taps[g - 1] + 1
        while k < taps[g] and vmcnt_of(ins[k]) is None:      # the wait behind the trip before
            k += 1
        while k < taps[g] and not is_vm_op(ins[k]):           # its arithmetic
            k += 1
        cuts.append(k)
    return [ins[a:b] for a, b in zip(cuts, cuts[1:] + [len(ins)])]


def analyse(asm_text):
    """One record per function that inlines the tracker's sweep: name, resources, its sample loops.  A loop of several samples per iteration gives one entry per
    trip (each held to the tap and wait verdicts on its own); `valu_per_sample` is the whole loop's vector-ALU count over the samples it handles."""
    out = []
    for mangled, body, info in split_functions(asm_text):
        name = pretty_name(mangled)
        if name is None:
            continue
        loops = []
        for head, ins in loops_of(body):
            whole = analyse_loop(ins)
            if whole["f64_fma"] < 27 or any(x.startswith("s_swappc") for x in ins):      # the 27 accumulations of H and b and no call: a loop over samples
                continue
            samples = max(1, sum(1 for s in ins if s.startswith("v_rcp_f64")))             # one projection (one f64 reciprocal) per sample
            valu = sum(whole["classes"][c] for c in VALU_CLASSES)
            trips = split_trips(ins)
            for t, part in enumerate(trips):
                a = whole if len(trips) == 1 else analyse_loop(part)
                a.update(header=head if len(trips) == 1 else "%s, trip %d of %d" % (head, t + 1, len(trips)), samples_in_loop=samples,
                         loop_instructions=len(ins), loop_valu=valu, valu_per_sample=valu / samples, lds_in_loop=whole["classes"]["LDS"])
                loops.append(a)
        out.append(dict(name=name, mangled=mangled, vgpr=info.get("NumVgprs"), sgpr=info.get("NumSgprs"), scratch=info.get("ScratchSize"), occupancy=info.get("Occupancy"),
                        lds=info.get("LDSByteSize"), hot=name in HOT, loops=loops, verdict=all(l["verdict"] is not False for l in loops),
                        prefetch_verdict=all(l["prefetch_verdict"] is not False for l in loops)))
    out.sort(key=lambda r: (not r["hot"], r["name"]))
    return out


def render(records, title):
    o = ["## " + title, ""]
    o.append("| function | VGPR | scratch B | occupancy | LDS B | VALU per sample | sample loops | taps before the first wait that covers one | nothing touches their registers until then | scratch in the loop | verdict | own requests a wait in front of the taps forces | verdict |")
    o.append("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in records:
        taps = ", ".join("%d of %d" % (l["taps_before_wait"], l["tap_loads"]) for l in r["loops"])
        unt = ", ".join({True: "yes", False: "NO", None: "-"}[l["dest_untouched"]] for l in r["loops"])
        scr = ", ".join(str(l["scratch_in_loop"]) for l in r["loops"])
        frc = ", ".join("-" if l["prefetch_verdict"] is None else "%d (%s)" % (l["prefetch_forced"], " ".join(w["wait"] for w in l["prefetch_waits"]) or "no wait") for l in r["loops"])
        vps = ", ".join(sorted(set("%g" % l["valu_per_sample"] for l in r["loops"]), key=float))
        o.append("| `%s`%s | %s | %s | %s | %s | %s | %d | %s | %s | %s | %s | %s | %s |" % (r["name"], " **(hot)**" if r["hot"] else "", r["vgpr"], r["scratch"], r["occupancy"] if r["occupancy"] is not None else "-",
                                                                     r["lds"] if r["lds"] is not None else "-", vps, len(r["loops"]), taps, unt, scr, "ok" if r["verdict"] else "**FAILS**", frc,
                                                                     "ok" if r["prefetch_verdict"] else "**FAILS**"))
    o.append("")
    for r in records:
        if not r["hot"]:
            continue
        for k, l in enumerate(r["loops"]):
            o.append("### `%s`, sample loop %d of %d (%s)" % (r["name"], k + 1, len(r["loops"]), l["header"]))
            o.append("")
            o.append("%d instructions per trip: " % l["instructions"] + ", ".join("%s %d" % (c, l["classes"][c]) for c in CLASSES if l["classes"][c]))
            o.append("")
            o.append("the loop handles %d sample(s) per iteration with %d instructions, %d of them vector ALU: %g VALU per sample"
                     % (l["samples_in_loop"], l["loop_instructions"], l["loop_valu"], l["valu_per_sample"]))
            o.append("")
            o.append("memory operations and waits in trip order: " + " -> ".join(l["memory_order"]))
            o.append("")
            o.append("verdict: %s (%d of %d tap loads in front of the first covering wait, %s; %d instructions between the last of them and that wait)"
                     % ("ok" if l["verdict"] else "FAILS", l["taps_before_wait"], l["tap_loads"], l["first_wait"], l.get("between_issue_and_wait", 0)))
            o.append("")
            o.append("waits between the trip's first memory request and its first tap load: %s -- verdict: %s"
                     % (", ".join("%s behind %d requests of the trip forces %d of them" % (w["wait"], w["issued"], w["forced"]) for w in l["prefetch_waits"]) or "none",
                        "ok" if l["prefetch_verdict"] else "FAILS"))
            o.append("")
    return "\n".join(o)


def run(rev=None, asm=None, src_root=None):
    """Records for the working tree (default), a git revision, another source tree or an assembly file."""
    if asm:
        return analyse(open(asm).read())
    hipcc = find_hipcc()
    if hipcc is None:
        raise RuntimeError("no hipcc")
    with tempfile.TemporaryDirectory(prefix="tracker_isa_") as tmp:
        root = checkout_rev(rev, tmp) if rev else (src_root or ROOT)
        return analyse(compile_asm(root, hipcc))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rev", help="analyse this git revision instead of the working tree")
    ap.add_argument("--asm", help="analyse this assembly file instead of compiling")
    ap.add_argument("--src-root", help="another checkout of the repository")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    rec = run(rev=a.rev, asm=a.asm, src_root=a.src_root)
    if a.json:
        print(json.dumps(rec, indent=1))
    else:
        print(render(rec, "tracker sample loops: " + (a.rev or a.asm or a.src_root or "working tree")))
    hot = [r for r in rec if r["hot"]]
    return 0 if len(hot) == len(HOT) and all(r["verdict"] and r["prefetch_verdict"] for r in hot) else 1


if __name__ == "__main__":
    sys.exit(main())
