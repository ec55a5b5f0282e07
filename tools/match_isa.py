#!/usr/bin/env python3
"""What the compiler made of the guided matcher's lean kernel (scavislam_amd/csrc/match.hip, match_kernel3).

Has csrc/Makefile write the gfx950 assembly of match.hip (build/match.s: the unit's own flags, device only) and reads match_kernel3 in layout order.  The
kernel's stages are found by their landmarks: the hit compaction of stage (3) is its ds_add_rtn_u32, the pixel-row requests of (3b) are the 8-byte loads
between the last of those and the f64 arithmetic of stage (4), which ends in front of the first v_dot4_u32_u8 (the key patch's texture sums); the later trips
of stage (5) are the loop that holds eight 8-byte loads and the dot products; the byte path of stage (2) is the run of blocks with single-byte or two-byte
loads, and quad_less the innermost loops that touch neither memory nor the LDS.  It prints, and holds the kernel to:

    no flat_* instruction: a flat request counts on lgkmcnt as well as vmcnt, so every wait for the LDS also waits for the pixel rows in flight;

    between the first row request of (3b) and the last f64 instruction of (4), no wait that covers a row: vmcnt(N) leaves the N youngest requests open, so
    it forces every row with N or more requests behind it; an lgkmcnt wait forces a row that was requested with a flat load.  The rows are requested there
    so that their round trip runs under the bilinear arithmetic -- a wait in between makes the two run one after the other;

    on the later trips of (5), all eight row requests in front of the first wait that covers one of them (one round trip per trip, not one per row);

    v_mad_u64_u32, v_mad_i64_i32 and v_mul_lo_u32 (quarter rate) only inside the byte path and quad_less;

    VGPR <= 64, no scratch, LDS <= 16 KB, 8 waves per SIMD.

tests/test_match_isa.py asserts these; profiles/match_isa.md holds the tables of both sides of the change that introduced the tool.

    python tools/match_isa.py                 # the working tree
    python tools/match_isa.py --rev HEAD~1    # another commit (git archive into a temporary directory)
    python tools/match_isa.py --asm match.s   # an assembly file made elsewhere
    python tools/match_isa.py --json          # the same as one JSON document
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracker_loop_isa as T  # noqa: E402  (the assembly reader: functions, blocks, instruction classes, wait counts)

KERNEL = "match_kernel3"
FORBIDDEN = ("v_mad_u64_u32", "v_mad_i64_i32", "v_mul_lo_u32")
CLASSES = T.CLASSES


def compile_asm(src_root, hipcc):
    """build/match.s by the Makefile's own rule: the Makefile alone knows the flags."""
    csrc = os.path.join(src_root, T.CSRC)
    r = subprocess.run(["make", "-C", csrc, "HIPCC=" + hipcc, "build/match.s"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if r.returncode != 0:
        raise RuntimeError("make build/match.s failed:\n" + r.stderr[-4000:])
    return open(os.path.join(csrc, "build", "match.s")).read()


def kernel_text(asm_text):
    """(body lines, resources) of match_kernel3."""
    m = re.search(r"^(_Z\w*%s\w*):\s*(;.*)?$" % KERNEL, asm_text, re.M)
    if not m:
        raise RuntimeError("no %s in the assembly" % KERNEL)
    end = asm_text.index(".Lfunc_end", m.end())
    body = asm_text[m.end():end].split("\n")
    tail = asm_text[end:end + 6000]
    nxt = re.search(r"^_Z\w+:", tail, re.M)
    tail = tail[:nxt.start()] if nxt else tail
    res = {}
    for key in ("NumVgprs", "NumSgprs", "ScratchSize", "Occupancy", "LDSByteSize"):
        mk = re.search(r"^; (?:Total)?%s: (\d+)" % key, tail, re.M)
        res[key] = int(mk.group(1)) if mk else None
    return body, res


def is_row(s):
    return re.match(r"^(global|flat)_load_dwordx2\s", s) is not None


def lgkmcnt_of(s):
    if not s.startswith("s_waitcnt"):
        return None
    m = re.search(r"lgkmcnt\((\d+)\)", s)
    if m:
        return int(m.group(1))
    m = re.match(r"^s_waitcnt\s+(0x[0-9a-fA-F]+|\d+)\s*$", s)      # a raw immediate: gfx9 lgkmcnt = bits 11:8
    if m:
        v = (int(m.group(1), 0) >> 8) & 0xf
        return v if v != 0xf else None
    return None


def covered_rows(ins, rows, p):
    """The row requests (indices into ins) that the wait at ins[p] forces to complete."""
    out = []
    n, lg = T.vmcnt_of(ins[p]), lgkmcnt_of(ins[p])
    for t in rows:
        if t >= p:
            continue
        if n is not None and sum(1 for q in range(t + 1, p) if T.is_vm_op(ins[q])) >= n:
            out.append(t)
        elif lg is not None and ins[t].startswith("flat_"):      # (lgkmcnt(N > 0) behind other LDS traffic may leave it open: counted as covered, the safe side)
            out.append(t)
    return out


def loops_with_members(blocks):
    """{header label: indices of the blocks of that loop, nested loops' blocks included (layout range)}."""
    direct = {}
    for k, b in enumerate(blocks):
        for h in (b["header"], b["label"]):
            if h and h.startswith(".L"):
                direct.setdefault(h, []).append(k)
    heads = set(b["header"] for b in blocks if b["header"])
    return {h: list(range(min(ks), max(ks) + 1)) for h, ks in direct.items() if h in heads}


def analyse(asm_text):
    body, res = kernel_text(asm_text)
    blocks = T.parse_blocks(body)
    seq = [(k, s) for k, b in enumerate(blocks) for s in b["ins"]]
    ins = [s for _, s in seq]
    blk = [k for k, _ in seq]
    ops = [s.split()[0] for s in ins]
    counts = dict.fromkeys(CLASSES, 0)
    for o in ops:
        counts[T.instr_class(o)] += 1
    flat = [s for s in ins if s.startswith("flat_")]
    rec = dict(kernel=KERNEL, vgpr=res["NumVgprs"], sgpr=res["NumSgprs"], scratch=res["ScratchSize"], occupancy=res["Occupancy"], lds=res["LDSByteSize"],
               instructions=len(ins), classes=counts, valu=sum(1 for o in ops if o.startswith("v_")), waits=sum(1 for o in ops if o == "s_waitcnt"),
               vmem=counts["VMEM"], flat=len(flat), flat_ops=sorted(set(s.split()[0] for s in flat)), barriers=sum(1 for o in ops if o == "s_barrier"))

    # ---- (3b) and (4)
    adds = [i for i, o in enumerate(ops) if o == "ds_add_rtn_u32"]
    if not adds:
        raise RuntimeError("no hit compaction (ds_add_rtn_u32) in %s" % KERNEL)
    first_dot = next(i for i in range(adds[-1], len(ops)) if ops[i] == "v_dot4_u32_u8")
    f64 = [i for i in range(adds[-1], first_dot) if "f64" in ops[i]]
    rows = [i for i in range(adds[-1], f64[0]) if is_row(ins[i])]
    pre = dict(rows=len(rows), f64=len(f64), waits=[])
    if rows:
        for p in range(rows[0] + 1, f64[-1] + 1):
            if ops[p] == "s_waitcnt":
                cov = covered_rows(ins, rows, p)
                in_flight = sum(1 for t in rows if t < p)
                pre["waits"].append(dict(wait=ins[p], rows_in_flight=in_flight, forced=len(cov), f64_behind=sum(1 for q in f64 if q > p)))
        pre["between"] = [ins[i].split()[0] for i in range(rows[0], f64[0]) if T.is_vm_op(ins[i])]
    pre["forced"] = max([w["forced"] for w in pre["waits"]] or [0])
    pre["verdict"] = bool(rows) and pre["forced"] == 0
    rec["prefetch"] = pre

    # ---- later trips of (5): the loop with eight row requests and the dot products
    later = None
    for h, ks in sorted(loops_with_members(blocks).items()):
        start = next(k for k in ks if blocks[k]["label"] == h)
        order = [k for k in ks if k >= start] + [k for k in ks if k < start]
        trip = [s for k in order for s in blocks[k]["ins"]]
        trows = [i for i, s in enumerate(trip) if is_row(s)]
        if len(trows) >= 8 and any(s.startswith("v_dot4_u32_u8") for s in trip):
            first_wait = next((p for p in range(trows[0] + 1, len(trip)) if trip[p].startswith("s_waitcnt") and covered_rows(trip, trows, p)), None)
            before = sum(1 for t in trows if first_wait is None or t < first_wait)
            mem = []
            for s in trip:
                if T.is_vm_op(s):
                    mem.append(s.split()[0])
                elif T.vmcnt_of(s) is not None and s.startswith("s_waitcnt") and "vmcnt" in s:
                    mem.append("vmcnt(%d)" % T.vmcnt_of(s))
            later = dict(header=h, rows=len(trows), rows_before_wait=before, first_wait=trip[first_wait] if first_wait is not None else None,
                         memory_order=mem, verdict=before == len(trows))
    rec["later_trips"] = later

    # ---- quarter-rate multiplies: where they stand
    allowed = set()
    small = [k for k, b in enumerate(blocks) if any(re.match(r"^(global|flat)_load_(u|s)(byte|short)", s) for s in b["ins"])]
    byte_blocks = set(range(min(small), max(small) + 1)) if small else set()
    allowed |= byte_blocks
    quad_blocks = set()
    for h, ks in loops_with_members(blocks).items():
        lins = [s for k in ks for s in blocks[k]["ins"]]
        if lins and not any(T.instr_class(s.split()[0]) in ("VMEM", "LDS") for s in lins):
            quad_blocks |= set(ks)
    allowed |= quad_blocks
    mul = {}
    for name in FORBIDDEN:
        idx = [i for i, o in enumerate(ops) if o.startswith(name)]
        mul[name] = dict(total=len(idx), byte_path=sum(1 for i in idx if blk[i] in byte_blocks), quad_less=sum(1 for i in idx if blk[i] in quad_blocks and blk[i] not in byte_blocks),
                         common_path=sum(1 for i in idx if blk[i] not in allowed))
    rec["multiplies"] = mul
    rec["multiplies_verdict"] = all(m["common_path"] == 0 for m in mul.values())
    rec["other_64bit"] = dict(v_lshl_add_u64=sum(1 for o in ops if o.startswith("v_lshl_add_u64")), v_ashrrev_i32_31=sum(1 for s in ins if re.match(r"^v_ashrrev_i32\w*\s+v\d+, 31,", s)))
    rec["resources_verdict"] = bool(res["NumVgprs"] is not None and res["NumVgprs"] <= 64 and res["ScratchSize"] == 0 and res["LDSByteSize"] is not None
                                    and res["LDSByteSize"] <= 16384 and res["Occupancy"] == 8)
    rec["verdict"] = bool(rec["flat"] == 0 and pre["verdict"] and later is not None and later["verdict"] and rec["multiplies_verdict"] and rec["resources_verdict"])
    return rec


def render(r, title):
    ok = lambda v: "ok" if v else "**FAILS**"      # noqa: E731
    o = ["## " + title, ""]
    o.append("| VGPR | SGPR | scratch B | LDS B | waves / SIMD | instructions | VALU | f64 | VMEM | s_waitcnt | flat |")
    o.append("|---|---|---|---|---|---|---|---|---|---|---|")
    o.append("| %s | %s | %s | %s | %s | %d | %d | %d | %d | %d | %d |" % (r["vgpr"], r["sgpr"], r["scratch"], r["lds"], r["occupancy"], r["instructions"], r["valu"], r["classes"]["f64"],
                                                                    r["vmem"], r["waits"], r["flat"]))
    o.append("")
    o.append("resources (VGPR <= 64, scratch 0, LDS <= 16384, 8 waves): %s" % ok(r["resources_verdict"]))
    o.append("")
    o.append("flat instructions: %d%s -- %s" % (r["flat"], " (" + ", ".join(r["flat_ops"]) + ")" if r["flat_ops"] else "", ok(r["flat"] == 0)))
    o.append("")
    p = r["prefetch"]
    o.append("(3b) -> (4): %d row requests, %d f64 instructions; memory requests from the first row to the first f64 instruction: %s" % (p["rows"], p["f64"], " -> ".join(p.get("between", [])) or "none"))
    o.append("")
    o.append("| wait between the first row request and the last f64 instruction | rows in flight | rows it forces | f64 instructions behind it |")
    o.append("|---|---|---|---|")
    for w in p["waits"]:
        o.append("| `%s` | %d | %d | %d |" % (w["wait"], w["rows_in_flight"], w["forced"], w["f64_behind"]))
    o.append("")
    o.append("no wait forces a row before the arithmetic is done: %s" % ok(p["verdict"]))
    o.append("")
    lt = r["later_trips"]
    if lt is None:
        o.append("later trips of (5): no loop with eight row requests found -- **FAILS**")
    else:
        o.append("later trips of (5) (%s): %s" % (lt["header"], " -> ".join(lt["memory_order"])))
        o.append("")
        o.append("%d of %d row requests in front of the first wait that covers one (`%s`): %s" % (lt["rows_before_wait"], lt["rows"], lt["first_wait"], ok(lt["verdict"])))
    o.append("")
    o.append("| quarter-rate multiply | in the kernel | byte path | quad_less | common path |")
    o.append("|---|---|---|---|---|")
    for name in FORBIDDEN:
        m = r["multiplies"][name]
        o.append("| `%s` | %d | %d | %d | %d |" % (name, m["total"], m["byte_path"], m["quad_less"], m["common_path"]))
    o.append("")
    o.append("none on the common path: %s (other 64-bit address arithmetic, not held: %d `v_lshl_add_u64`, %d sign extensions)"
             % (ok(r["multiplies_verdict"]), r["other_64bit"]["v_lshl_add_u64"], r["other_64bit"]["v_ashrrev_i32_31"]))
    o.append("")
    return "\n".join(o)


def run(rev=None, asm=None, src_root=None):
    """The record for the working tree (default), a git revision, another source tree or an assembly file."""
    if asm:
        return analyse(open(asm).read())
    hipcc = T.find_hipcc()
    if hipcc is None:
        raise RuntimeError("no hipcc")
    with tempfile.TemporaryDirectory(prefix="match_isa_") as tmp:
        root = T.checkout_rev(rev, tmp) if rev else (src_root or T.ROOT)
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
        print(render(rec, "match_kernel3: " + (a.rev or a.asm or a.src_root or "working tree")))
    return 0 if rec["verdict"] else 1


if __name__ == "__main__":
    sys.exit(main())
