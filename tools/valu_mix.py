#!/usr/bin/env python3
"""Issue-cost model of the sweep kernels' VALU instruction mix.

The sweep is VALU-issue-bound, so its roofline peak is the SIMDs' issue rate
for ITS instruction mix, not a constant per instruction.  This tool:

  1. compiles ksched_kernels.hip for gfx950 (device code only) and
     disassembles it with llvm-objdump;
  2. for every sweep_kernel<NPL, EXT, LWU> instance takes its per-pod loop
     (the longest backward branch: the loop over the pods of a sweep block,
     nested clause loops counted once) and histograms its VALU opcodes.  The
     resource-only kernels take the pods in batches of WL_T (ksched_dev.hpp):
     their longest backward branch is the loop over the batches, the longest
     one inside it the pod loop, and what the outer loop holds besides is the
     batch step, which runs once per WL_T pods.  loop_valu is VALU per pod
     there: the pod loop's body (pod_valu) + the batch step's (batch_valu) /
     WL_T, and the costs are weighted alike.  The default strategy's
     resource-only kernels recompute a node's cpu terms only where the pod's
     cpu key changes: their pod loop is priced as the hit path (pod_valu) +
     miss_rate x the cpu block (cpu_block_valu), with the miss rate a
     parameter (--miss-rate, default MISS_RATE) recorded in the JSON.  Their
     pod loop holds the pod's body once per descriptor register set (two,
     taken in turn): counts are per pod, a turn's divided by pods_per_turn,
     and the clamp that only zero requests run is left out;
  3. prices each opcode with the issue cost measured on MI355X at 4 waves per
     SIMD by tools/valu_issue.hip (profiles/valu_issue.jsonl); an opcode the
     microbenchmark does not cover takes its class's median (VOP1/VOP2
     32-bit moves / adds / logic ops: the 2-cycle class; everything else the
     4-cycle class), and the covered share is reported;
  4. writes profiles/valu_mix.json: per kernel the cost-weighted cycles per
     VALU wave-instruction, keyed by the hash bench.py uses for the kernel
     sources.

bench.py then prices the sweep at peak = 256 CUs x 4 SIMDs x 2.4 GHz /
(cycles per VALU instruction) wave-instructions per second.

  python3 tools/valu_mix.py            (no GPU needed; llvm-objdump from ROCm)
"""
from __future__ import annotations

import collections
import hashlib
import json
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "k8s-1m_amd" / "csrc"
# the hash bench.py keys its per-configuration measurements by (bench.KERNEL_SOURCES)
def bench_kernel_sources(root):
    """bench.py's KERNEL_SOURCES, read from its text (one list for every hash)."""
    import ast
    tree = ast.parse((root / "bench.py").read_text())
    for node in tree.body:
        if isinstance(node, ast.Assign) and any(getattr(t, "id", None) == "KERNEL_SOURCES" for t in node.targets):
            return ast.literal_eval(node.value)
    raise RuntimeError("bench.py has no KERNEL_SOURCES")


KERNEL_SOURCES = bench_kernel_sources(ROOT)
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
HIPCC = "/opt/rocm/bin/hipcc"
# Pods of a sweep block whose cpu key (req_cpu, nz_cpu) differs from the
# previous pod's, per pod swept: they run the pod loop's cpu block.
# 1 - ks_debug_counters [9] / [2] over a C3 run (bench.py --steps 20 --warmup 5)
MISS_RATE = 0.345
WAVES = 4  # the sweep's occupancy: 4 waves per SIMD (5 for the EXT kernels; the costs barely differ)
FAST = re.compile(r"^v_(add|sub|subrev|and|or|xor|not|mov|ashrrev|lshrrev)_(u32|i32|b32|f32)(_e32|_e64)?$|"
                  r"^v_(add|mul)_f32(_e32)?$")


def kernel_src_hash() -> str:
    h = hashlib.sha256()
    for f in KERNEL_SOURCES:
        h.update((ROOT / f).read_bytes())
    return h.hexdigest()[:16]


def load_costs(path: Path):
    costs = {}
    for ln in path.read_text().splitlines():
        if not ln.startswith("{"):
            continue
        r = json.loads(ln)
        if r["waves_per_simd"] == WAVES:
            costs[r["instr"]] = r["cycles_per_instr"]
    return costs


def disassemble() -> list[str]:
    with tempfile.TemporaryDirectory() as d:
        obj = Path(d) / "k.o"
        subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-ffp-contract=off",
                        f"-I{ROOT / 'include'}", f"-I{CSRC}", "--cuda-device-only", "--no-gpu-bundle-output",
                        "-c", str(CSRC / "ksched_kernels.hip"), "-o", str(obj)], check=True)
        out = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", str(obj)], check=True, capture_output=True,
                             text=True).stdout
    return out.splitlines()


def kernels(lines):
    """{mangled name: [(address, opcode, operands)]} for the sweep kernels."""
    out, cur = {}, None
    for ln in lines:
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", ln)
        if m:
            cur = m.group(1) if "sweep_kernel" in m.group(1) and not general_variant(m.group(1)) else None
            if cur:
                out[cur] = []
            continue
        if cur:
            m = re.match(r"^\s*([a-z_0-9]+)(.*?)//\s*([0-9A-F]+):", ln)
            if m:
                out[cur].append((int(m.group(3), 16), m.group(1), m.group(2).strip()))
    return out


def batch_pods() -> int:
    """WL_T of ksched_dev.hpp: the pods of one batch step."""
    m = re.search(r"constexpr int WL_T = (\d+);", (CSRC / "ksched_dev.hpp").read_text())
    return int(m.group(1))


def pod_loop(ins, within=None):
    """[lo, hi) of the longest backward branch's loop (within: strictly inside that range)."""
    best = None
    for a, op, args in ins:
        if within and not (within[0] <= a < within[1]):
            continue
        if not (op.startswith("s_cbranch") or op == "s_branch"):
            continue
        m = re.match(r"^(-?\d+)", args)
        if not m:
            continue
        off = int(m.group(1))
        if off >= 32768:
            off -= 65536
        if off >= 0:
            continue
        t = a + 4 + 4 * off
        if within and (t <= within[0] or a + 4 >= within[1]):
            continue
        if best is None or a - t > best[1] - best[0]:
            best = (t, a + 4)
    return best


KEY_CMP = re.compile(r"^s_cmp_(eq|lg)_u64$")
SGPR_PAIRS = re.compile(r"^s\[\d+:\d+\], s\[\d+:\d+\]$")
COND = ("s_cbranch_vccz", "s_cbranch_vccnz", "s_cbranch_scc0", "s_cbranch_scc1")


def branch_target(a, args):
    off = int(re.match(r"^(-?\d+)", args).group(1))
    return a + 4 + 4 * (off - 65536 if off >= 32768 else off)


def cpu_block(ins, outer, inner):
    """The pod loop's conditional block: the resource-only kernels
    of the default strategy keep each node's cpu terms while the pod's cpu key
    (req_cpu, nz_cpu) stays, and recompute them behind a wave-uniform branch on
    a compare of two SGPR pairs.  The loop holds one copy of the pod's body per
    descriptor register set (two, taken in turn), so a turn of the
    loop is that many pods and that many such branches.  One turn is walked
    from the first of them with all of them taken, and one with none taken;
    the turn with fewer VALU instructions is the hit path.  The loop's own
    backward branch is taken.  A conditional branch over nothing but the
    clamp of the BalancedAllocation fractions (v_max_f64 / v_min_f64 and
    scalar instructions) is taken too: the clamp runs for zero requests only
    and is not priced.  Other conditional branches fall through: they leave
    the loop or skip a load; s_cbranch_exec* never jump, the wave is whole.
    Returns (hit addresses, miss-only addresses, pods per turn), or None
    without such a branch (every other kernel)."""
    body = [(a, op, args) for a, op, args in ins if inner[0] <= a < inner[1]]
    # (a turn may re-enter a few scalar moves above the longest branch's target)
    lo = min([inner[0]] + [branch_target(a, args) for a, op, args in body
                           if op == "s_branch" and outer[0] <= branch_target(a, args)])
    body = [(a, op, args) for a, op, args in ins if lo <= a < inner[1]]
    at = {a: i for i, (a, _, _) in enumerate(body)}
    keys = []
    for i, (a, op, args) in enumerate(body):
        if KEY_CMP.match(op) and SGPR_PAIRS.match(args) and (not keys or i > keys[-1]):
            k = next((j for j in range(i + 1, len(body)) if body[j][1] in COND), None)
            if k is not None:
                keys.append(k)
    if not keys:
        return None
    key = keys[0]

    def over_clamp_only(i):
        a, op, args = body[i]
        j = at.get(branch_target(a, args)) if op in COND else None
        if j is None or j <= i + 1:
            return False
        ops = [body[k][1] for k in range(i + 1, j)]
        return any(o.startswith("v_min_f64") for o in ops) and all(
            o.startswith(("v_max_f64", "v_min_f64", "s_")) and not o.startswith(("s_cbranch", "s_branch")) for o in ops)

    def turn(taken):
        seen, i = [], key
        while True:
            a, op, args = body[i]
            if i == key and seen:
                return seen
            seen.append(a)
            jump = (op == "s_branch" or (i in keys and taken) or (i == len(body) - 1 and op in COND) or
                    over_clamp_only(i))
            nxt = at.get(branch_target(a, args)) if jump else i + 1
            if nxt is None or nxt >= len(body) or len(seen) > len(body):
                raise RuntimeError("the pod loop's turn leaves the loop")
            i = nxt

    valu = lambda path: sum(1 for a in path if body[at[a]][1].startswith("v_"))
    p, q = turn(True), turn(False)
    hit, miss = (p, q) if valu(p) <= valu(q) else (q, p)
    return set(hit), set(miss) - set(hit), len(keys)


def general_variant(mangled: str) -> bool:
    """sweep_kernel<NPL, EXT, LWU, GF != 0>: the instances of a non-default
    NodeResourcesFit strategy, which bench.py never runs."""
    return re.search(r"sweep_kernelILi\d+ELb\dELi\d+ELi[1-9]\d*EE", mangled) is not None


def template_args(mangled: str) -> str:
    m = re.search(r"sweep_kernelILi(\d+)ELb(\d)ELi(\d+)E", mangled)
    return f"<{m.group(1)}, {'true' if m.group(2) == '1' else 'false'}, {m.group(3)}>"


SGPR_SRC = re.compile(r"^(s\d|s\[|vcc|exec|m0)")


def cost_of(op: str, costs: dict, fast_med: float, slow_med: float, args: str = ""):
    # the 2-cycle class needs VGPR (or inline-constant) sources: with an SGPR
    # source it issues like the 4-cycle class (tools/valu_issue.hip "(s, v)"
    # rows, profiles/r4/valu_vop.jsonl)
    if FAST.match(op) and any(SGPR_SRC.match(x.strip()) for x in args.split(",")[1:]):
        return slow_med, "v_add_u32 (s, v)" in costs
    base = re.sub(r"_e(32|64)$", "", op)
    for k in (op, base, base.replace("_dpp", "") + "_dpp" if op.endswith("_dpp") else base):
        if k in costs:
            return costs[k], True
    if base.startswith("v_cmp"):
        for k in costs:
            if k.startswith("v_cmp") and k.split("_")[-1] == base.split("_")[-1]:
                return costs[k], True
    return (fast_med if FAST.match(op) else slow_med), False


def main():
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--miss-rate", type=float, default=MISS_RATE,
                    help="share of swept pods whose cpu key differs from their predecessor's")
    miss_rate = ap.parse_args().miss_rate
    costs = load_costs(ROOT / "profiles" / "valu_issue.jsonl")
    fast = sorted(v for k, v in costs.items() if FAST.match(k))
    slow = sorted(v for k, v in costs.items() if not FAST.match(k) and v < 8)
    fast_med, slow_med = fast[len(fast) // 2], slow[len(slow) // 2]
    res = {"kernel_src": kernel_src_hash(), "waves_per_simd": WAVES, "source": "profiles/valu_issue.jsonl",
           "class_median": {"fast_32bit": fast_med, "other": slow_med}, "kernels": {}}
    T = batch_pods()
    for name, ins in kernels(disassemble()).items():
        lo, hi = pod_loop(ins)
        targs = template_args(name)
        batched = ", false," in targs
        inner = pod_loop(ins, (lo, hi)) if batched else None
        if batched and inner is None:
            raise RuntimeError(f"{targs}: no pod loop inside the loop over the batches")
        blk = cpu_block(ins, (lo, hi), inner) if batched else None
        miss_only = blk[1] if blk else set()
        turn_pods = blk[2] if blk else 1  # copies of the pod's body in the pod loop
        on_path = (blk[0] | blk[1]) if blk else None
        # (opcode, operands, weight): the batch step's instructions run once per
        # T pods, the cpu block's once per miss_rate pods; a turn of the pod
        # loop is turn_pods pods, and what no turn reaches (the clamp) has no weight
        def weight(a):
            if not batched or not (inner[0] <= a < inner[1]):
                return 1.0 / T if batched else 1.0
            if on_path is not None and a not in on_path:
                return 0.0
            return (miss_rate if a in miss_only else 1.0) / turn_pods
        loop = [(op, args, weight(a)) for a, op, args in ins if lo <= a < hi and op.startswith("v_") and weight(a) > 0]
        in_batch = lambda a: batched and not (inner[0] <= a < inner[1])
        hist = collections.Counter(op for a, op, _ in ins
                                   if lo <= a < hi and op.startswith("v_") and not in_batch(a) and a not in miss_only and
                                   (on_path is None or a in on_path))
        mhist = collections.Counter(op for a, op, _ in ins if a in miss_only and op.startswith("v_"))
        bhist = collections.Counter(op for a, op, _ in ins if lo <= a < hi and op.startswith("v_") and in_batch(a))
        n = sum(w for _, _, w in loop)
        cyc = covered = 0.0
        for op, args, w in loop:
            v, ok = cost_of(op, costs, fast_med, slow_med, args)
            cyc += v * w
            covered += w if ok else 0
        k = {"mangled": name, "loop_valu": round(n, 2) if batched else int(n),"cycles_per_valu": round(cyc / n, 4),
             "measured_share": round(covered / n, 4),
             "hist": dict(hist.most_common())}
        if batched:
            k.update(pod_valu=sum(hist.values()) / turn_pods, batch_valu=sum(bhist.values()), batch_pods=T,
                     batch_hist=dict(bhist.most_common()), pods_per_turn=turn_pods)
        if blk:
            # pod_valu: the hit path; a pod whose cpu key differs from its
            # predecessor's adds cpu_block_valu
            k.update(cpu_block_valu=sum(mhist.values()) / turn_pods, miss_rate=miss_rate,
                     cpu_block_hist=dict(mhist.most_common()))
        res["kernels"][targs] = k
    out = ROOT / "profiles" / "valu_mix.json"
    out.write_text(json.dumps(res, indent=1) + "\n")
    for k, v in sorted(res["kernels"].items()):
        parts = f" = {v['pod_valu']:g} + {v['batch_valu']} / {v['batch_pods']}" if "pod_valu" in v else ""
        if "cpu_block_valu" in v:
            parts += f" + {v['miss_rate']} x {v['cpu_block_valu']:g}"
        print(f"sweep_kernel{k}: {v['loop_valu']}{parts} VALU per pod in the pod loop, {v['cycles_per_valu']} cycles each "
              f"(measured opcodes {v['measured_share']:.0%})")
    print("->", out.relative_to(ROOT))


if __name__ == "__main__":
    sys.exit(main())
