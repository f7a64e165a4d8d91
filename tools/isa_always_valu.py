#!/usr/bin/env python
"""VALU instructions a wave of one kernel cannot avoid issuing, per phase (no GPU needed).  The file is compiled to a listing with the
flags csrc/Makefile gives it (makefile_flags.py), the kernel is cut at its first label (entry) and at s_barrier, and in each phase
the VALU instructions are counted twice: all of them, and those outside every region that a forward conditional branch can skip
(the innermost forward branch round a loop is the loop's guard, and a forward branch out of a loop is its exit: neither skips
anything, and a loop body counts once, per iteration; blocks laid out behind s_endpgm are only ever branched to and count as
skippable).  Also: `v_mov_b32 vN, 0` whose destination is next written by a DPP move with full row and bank masks — a zeroed
`old` operand that no lane can read.
  python tools/isa_always_valu.py mppi_rollout mppi_rollout_fusedILi2ELi8ELi1ELi2E [--tree other-checkout] [--listing file.s]
tests/test_mppi_dead_valu_isa.py uses the functions below."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from makefile_flags import per_file_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def listing(stem, root=ROOT):
    """hipcc -S of <root>/.../csrc/<stem>.hip under csrc/Makefile's flags for that file, as lines."""
    csrc = os.path.join(root, "ros-turtlebot-navigation_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, stem + ".s")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-fast-math", f"-I{root}/include", f"-I{csrc}",
                        *per_file_flags(stem), "-S", "--cuda-device-only", os.path.join(csrc, stem + ".hip"), "-o", out],
                       check=True, stderr=subprocess.DEVNULL)
        return open(out).read().split("\n")


def kernel_body(lines, pattern):
    """Instruction and label lines of the one kernel whose mangled name contains `pattern`, from its aligned entry on."""
    names = [m.group(1) for l in lines for m in [re.match(r"^(_Z\S+):", l)] if m and pattern in m.group(1)]
    assert len(names) == 1, (pattern, names)
    start = lines.index(names[0] + ":") if names[0] + ":" in lines else next(i for i, l in enumerate(lines) if l.startswith(names[0] + ":"))
    end = next(i for i in range(start, len(lines)) if ".Lfunc_end" in lines[i])
    body = [l.split(";")[0].rstrip() for l in lines[start + 1:end]]
    body = [l.strip() for l in body if l.strip() and (not l.strip().startswith(".") or re.match(r"^\.LBB\d+_\d+:", l.strip()))]
    # kernel-argument preload: a prologue for firmware that does not preload comes first and branches to the aligned entry
    for i, l in enumerate(body[:12]):
        if re.match(r"s_branch\s+\.LBB\d+_0\b", l):
            body = body[body.index(l.split()[1] + ":", i):]
            break
    return body


def _label(l):
    m = re.match(r"^(\.LBB\d+_\d+):", l)
    return m.group(1) if m else None


def _branch(l):
    m = re.match(r"^s_(c?)branch\S*\s+(\.LBB\d+_\d+)", l)
    return (bool(m.group(1)), m.group(2)) if m else None


def skippable(body):
    """One flag per line of `body`: can a forward conditional branch jump over it (see the module text)."""
    at = {_label(l): i for i, l in enumerate(body) if _label(l)}
    last = next((i for i, l in enumerate(body) if l.startswith("s_endpgm")), len(body))
    loops = [(at[b[1]], i) for i, l in enumerate(body) for b in [_branch(l)] if b and b[1] in at and at[b[1]] <= i]
    fwd = [(i, at[b[1]]) for i, l in enumerate(body) for b in [_branch(l)] if b and b[0] and b[1] in at and i < at[b[1]] <= last]
    guards = set()
    for lo, hi in loops:
        round_it = [(p, q) for p, q in fwd if p < lo and hi < q]
        if round_it:
            guards.add(max(round_it))   # the innermost: the one that starts last
    exits = {(p, q) for p, q in fwd for lo, hi in loops if lo <= p <= hi < q}   # leaves a loop: what follows is not jumped over
    skip = [i > last for i in range(len(body))]
    for p, q in fwd:
        if (p, q) not in guards and (p, q) not in exits:
            for i in range(p + 1, q):
                skip[i] = True
    return skip


def phases(body):
    """[(name, first, end)]: entry (to the first label behind the entry's own), up to s_barrier, after it."""
    labels = [i for i, l in enumerate(body) if _label(l)]
    first = labels[1] if _label(body[0]) else labels[0]
    bar = next((i for i, l in enumerate(body) if l.startswith("s_barrier")), len(body))
    return [("entry", 0, first), ("to barrier", first, bar), ("after barrier", bar, len(body))]


def count(body, op_prefix="v_"):
    """{phase: (all, always)} of the instructions whose mnemonic starts with op_prefix."""
    skip = skippable(body)
    out = {}
    for name, a, b in phases(body):
        hit = [i for i in range(a, b) if body[i].startswith(op_prefix)]
        out[name] = (len(hit), sum(1 for i in hit if not skip[i]))
    return out


def _dest(l):
    """First register of the destination operand of a VALU line, and how many registers it covers."""
    m = re.match(r"^v_\S+\s+v(\d+)\b", l) or re.match(r"^v_\S+\s+v\[(\d+):(\d+)\]", l)
    if not m:
        return None
    lo = int(m.group(1))
    return (lo, int(m.group(2)) if m.lastindex == 2 else lo)


def dead_zero_moves(body):
    """Indices of `v_mov_b32 vN, 0` whose vN is next written, in the same basic block, by a full-mask DPP move."""
    out = []
    for i, l in enumerate(body):
        m = re.match(r"^v_mov_b32_e32\s+v(\d+),\s*0$", l)
        if not m:
            continue
        n = int(m.group(1))
        for k in body[i + 1:]:
            if _label(k) or _branch(k):
                break
            d = _dest(k)
            if d and d[0] <= n <= d[1]:
                if k.startswith("v_mov_b32_dpp") and "row_mask:0xf" in k and "bank_mask:0xf" in k:
                    out.append(i)
                break
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    opt = {}
    for o in ("--tree", "--listing"):
        if o in args:
            i = args.index(o)
            opt[o] = args[i + 1]
            del args[i:i + 2]
    stem, kernel = args
    lines = open(opt["--listing"]).read().split("\n") if "--listing" in opt else listing(stem, opt.get("--tree", ROOT))
    body = kernel_body(lines, kernel)
    print(f"{kernel}: VALU per phase, all / outside every forward-skippable region")
    for (name, (n_all, n_always)), (_, (r_all, r_always)) in zip(count(body).items(), count(body, "v_rndne_f64").items()):
        print(f"  {name:14s} {n_all:4d} / {n_always:4d}    v_rndne_f64 {r_all} / {r_always}")
    dz = dead_zero_moves(body)
    dpp = sum(1 for l in body if l.startswith("v_mov_b32_dpp"))
    ph = phases(body)
    per = {name: sum(1 for i in dz if a <= i < b) for name, a, b in ph}
    print(f"  zero moves feeding a full-mask DPP move: {len(dz)} {per}   (DPP moves: {dpp}, v_mov_b32 v, 0: "
          f"{sum(1 for l in body if re.match(r'^v_mov_b32_e32 v[0-9]+, 0$', l))})")
