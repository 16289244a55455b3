#!/usr/bin/env python3
"""What stands between the barriers of a kernel's main loop, read from its assembly (works without a GPU):
   python tools/main_loop_waits.py lets_face_it_amd/csrc/lfi_pgemm.hip [name filter] [-- extra hipcc flags]
   python tools/main_loop_waits.py --asm unit.s [name filter]        (an assembly file made earlier)
Compiles the unit to device assembly with the Makefile's flags (make -s print-flags) and, for every kernel whose demangled name
contains the filter, prints one line per span that ends in an s_barrier of the MAIN LOOP - the basic blocks of the loops (as the
compiler's own "Loop Header" / "in Loop: Header=" comments on the block labels name them) that hold both a barrier and an MFMA; a
loop nested inside another is taken alone - as instruction classes in program order, run-length coded:
   nDMA  LDS-DMA (buffer_load / global_load ... lds)          nM    MFMA
   nlr   LDS read (ds_read*, ds_load*)                        nlw   LDS write
   nvl / nvs  other vector-memory loads / stores              nSCR  scratch_load / scratch_store
   vm(n) lgkm(n)  every s_waitcnt with its counts             .     anything else is left out (VALU, SALU, branches)
Flags: a vmcnt(0) or a scratch access inside the main loop ("!! vmcnt(0)", "!! scratch"). The ring kernels of this project keep
DMA in flight across their barriers with counted waits; a vmcnt(0) in the loop drains the ring, and scratch loads share the counter.
A kernel without a barrier inside a loop gets the one line "no barrier loop"."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def unit_asm(src, extra):
    """device assembly of one unit, compiled as the Makefile compiles it"""
    flags = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "lets_face_it_amd", "csrc"), "print-flags", "SRC=" + os.path.basename(src)],
                           capture_output=True, text=True, check=True).stdout.split()
    cmd = ["hipcc"] + flags + extra + ["--cuda-device-only", "-S", src, "-o", "-"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit("main_loop_waits: hipcc failed on %s" % src)
    return r.stdout


def demangle(names):
    if not names:
        return {}
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        out = names
    res = {}
    for m, d in zip(names, out):
        d = re.sub(r"\(anonymous namespace\)::", "", d)
        d = re.sub(r"^void ", "", d)
        res[m] = re.sub(r"\(.*$", "", d)
    return res


def kernels_of(asm):
    """-> [(mangled name, [instruction / label lines], {index of a label line: the compiler's comments on it})] of every kernel"""
    kern = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, re.M))
    res, cur, body, notes, fresh = [], None, None, None, False
    for line in asm.splitlines():
        s, _, com = line.partition(";")
        s = s.strip()
        if not s:
            if cur is not None and fresh and com:   # a comment line right under a label: more about that block
                notes[len(body) - 1] += " " + com
            continue
        m = re.match(r"^([A-Za-z_.$][\w.$]*):$", s)
        if m and m.group(1) in kern:
            cur, body, notes, fresh = m.group(1), [], {}, False
            res.append((cur, body, notes))
            continue
        if cur is None:
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if s.startswith(".") and not s.endswith(":"):
            continue   # directives
        body.append(s)
        fresh = s.endswith(":")
        if fresh:
            notes[len(body) - 1] = com
    return res


def classify(ins):
    op = ins.split()[0]
    if op == "s_waitcnt":
        parts = []
        for name, short in (("vmcnt", "vm"), ("lgkmcnt", "lgkm"), ("expcnt", "exp")):
            m = re.search(name + r"\((\d+)\)", ins)
            if m:
                parts.append("%s(%s)" % (short, m.group(1)))
        if not parts:   # a raw immediate: decode gfx9's fields (vmcnt 3:0 + 15:14, expcnt 6:4, lgkmcnt 11:8)
            m = re.search(r"s_waitcnt\s+(0x[0-9a-fA-F]+|\d+)", ins)
            if m:
                v = int(m.group(1), 0)
                vm, lg = (v & 15) | ((v >> 14) & 3) << 4, (v >> 8) & 15
                if vm != 63:
                    parts.append("vm(%d)" % vm)
                if lg != 15:
                    parts.append("lgkm(%d)" % lg)
        return "wait", " ".join(parts)
    if op == "s_barrier":
        return "barrier", None
    if op.startswith("scratch_"):
        return "SCR", None
    if op.startswith("v_mfma") or op.startswith("v_smfmac"):
        return "M", None
    if op.startswith(("buffer_load", "global_load")) and re.search(r"\blds\b", ins):
        return "DMA", None
    if op.startswith(("ds_read", "ds_load")):
        return "lr", None
    if op.startswith(("ds_write", "ds_store")):
        return "lw", None
    if op.startswith(("buffer_load", "global_load", "flat_load")):
        return "vl", None
    if op.startswith(("buffer_store", "global_store", "flat_store", "buffer_atomic", "global_atomic", "flat_atomic")):
        return "vs", None
    return None, None


def main_loop_lines(body, notes):
    """indices (program order) of the lines of the main loop's blocks, or None"""
    groups, cur = {}, None   # innermost loop header -> line indices of its blocks
    for i, s in enumerate(body):
        if s.endswith(":"):
            note = notes.get(i, "")
            m = re.search(r"in Loop: Header=(BB\d+_\d+)", note)
            cur = s[:-1] if "Loop Header" in note else (".L" + m.group(1) if m else None)
            continue
        if cur is not None:
            groups.setdefault(cur, []).append(i)
    lines = []
    for idx in groups.values():
        cls = set(classify(body[i])[0] for i in idx)
        if "barrier" in cls and "M" in cls:
            lines += idx
    return sorted(lines) or None


def spans_of(body, notes):
    """-> (lines of text, flags) for one kernel"""
    idx = main_loop_lines(body, notes)
    if idx is None:
        return ["no barrier loop"], []
    lines, flags, cur, run = [], set(), [], [None, 0]

    def flush_run():
        if run[0] is not None:
            cur.append(("%d%s" % (run[1], run[0])) if run[1] > 1 else run[0])
        run[0], run[1] = None, 0

    for s in (body[i] for i in idx):
        cls, txt = classify(s)
        if cls is None:
            continue
        if cls == "barrier":
            flush_run()
            lines.append(" ".join(cur) + "  | barrier")
            cur = []
            continue
        if cls == "wait":
            flush_run()
            if txt:
                cur.append(txt)
                if re.search(r"vm\(0\)", txt):
                    flags.add("vmcnt(0)")
            continue
        if cls == "SCR":
            flags.add("scratch")
        if run[0] == cls:
            run[1] += 1
        else:
            flush_run()
            run[0], run[1] = cls, 1
    return lines, sorted(flags)


def analyse(asm, flt=""):
    """-> [(demangled kernel name, [span lines], [flags])] for the kernels whose name contains flt"""
    kerns = kernels_of(asm)
    names = demangle([k for k, _, _ in kerns])
    res = []
    for k, body, notes in kerns:
        name = names.get(k, k)
        if flt and flt not in name:
            continue
        lines, flags = spans_of(body, notes)
        res.append((name, lines, flags))
    return res


def main():
    args = sys.argv[1:]
    extra = []
    if "--" in args:
        i = args.index("--")
        args, extra = args[:i], args[i + 1:]
    if args and args[0] == "--asm":
        with open(args[1]) as f:
            asm = f.read()
        args = args[1:]
    elif args:
        asm = unit_asm(args[0], extra)
    else:
        raise SystemExit(__doc__)
    flt = args[1] if len(args) > 1 else ""
    bad = 0
    for name, lines, flags in analyse(asm, flt):
        print(name + ("    !! " + ", ".join(flags) if flags else ""))
        prev, rep = None, 0
        for ln in lines + [None]:   # identical consecutive spans are printed once with a count
            if ln == prev:
                rep += 1
                continue
            if prev is not None:
                print("    " + (("%d x  " % rep) if rep > 1 else "") + prev)
            prev, rep = ln, 1
        bad += 1 if flags else 0
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
