"""Where k_pyr_stream's worker waves fetch their task descriptors, read off the gfx950 ISA (CPU box: hipcc --cuda-device-only -S, no GPU).

A worker wave requests the 64-byte descriptor of its NEXT task with a hand-placed `s_load_dwordx16` (pyr_stream.hip.h, PYR_DESC_FETCH) after the
current task's LDS reads have returned and before its arithmetic, and retires it with a hand-placed `s_waitcnt lgkmcnt(0)` behind the task's
stores.  The compiler's wait insertion does not know about that load, and the point of the placement -- the round trip to the scalar cache / L2
runs beside the task's ~100 vector instructions instead of in front of the next task -- is a property of the emitted code, not of the source
order (left to the compiler, the load sank below the task's last store).  The walk below follows every path of the worker code with "the
registers of a descriptor in flight" as its state and pins:
  * at every v_dot2_u32_u16 (horizontal pass) a descriptor is in flight: the fetch is issued before the task's first one;
  * at every v_ashr_pk_u8_i32 (end of a vertical pass) it still is: no `s_waitcnt lgkmcnt(0)` retires it before the task's last one;
  * nothing reads or writes the registers of a descriptor in flight (only a full lgkmcnt wait retires it: scalar loads return out of order);
  * the worker code holds no vector global load (a wave's vector memory operations retire in order: a wait for such a load would also wait
    for every pyramid store before it -- that is what the loader wave is for).
"""
import re
import shutil
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not Path("/opt/rocm/bin/hipcc").exists(), reason="hipcc not installed")

_SREG = re.compile(r"\bs(\d+)\b|\bs\[(\d+):(\d+)\]")
_VLOAD = re.compile(r"^(global_load|buffer_load|flat_load|scratch_load|global_atomic|buffer_atomic|flat_atomic)")
FETCH = "s_load_dwordx16"


def _sregs(text):
    out = set()
    for m in _SREG.finditer(text):
        if m.group(1):
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def _waits_all_lgkm(args):
    """does this s_waitcnt wait for lgkmcnt == 0?"""
    m = re.search(r"lgkmcnt\((\d+)\)", args)
    if m:
        return int(m.group(1)) == 0
    if re.fullmatch(r"(0x[0-9a-f]+|\d+)", args):   # raw immediate: lgkmcnt = bits 11:8 (gfx9)
        return ((int(args, 0) >> 8) & 0xf) == 0
    return False


@pytest.fixture(scope="module")
def worker():
    """(instructions, labels, index of the worker code's first descriptor load, the worker code) of k_pyr_stream.  The worker code = the
    instructions from which a descriptor fetch can still be reached: the wave's start-up and its task loop.  (Behind the loop the structured
    control flow falls through the `is this the loader wave` test, which a walk that does not evaluate conditions would follow.)"""
    import isa_vmem_check as chk
    kernels = chk.split_kernels(chk.compile_unit("orbx_extractor.hip"))
    names = [k for k in kernels if "k_pyr_stream" in k]
    assert len(names) == 1, names
    ins, labels, _ = kernels[names[0]]
    first = next(i for i, (op, _) in enumerate(ins) if op == FETCH)   # the loader wave and the shared prologue never load 64 bytes at once
    pred = {}
    for pc, (op, args) in enumerate(ins):
        for nx in _succ(ins, labels, pc):
            pred.setdefault(nx, []).append(pc)
    region, work = set(), [pc for pc, (op, _) in enumerate(ins) if op == FETCH]
    while work:
        pc = work.pop()
        if pc not in region:
            region.add(pc)
            work.extend(pred.get(pc, []))
    return ins, labels, first, region


def _succ(ins, labels, pc):
    op, args = ins[pc]
    if op in ("s_endpgm", "s_trap"):
        return []
    if op == "s_branch":
        return [labels[args.split()[0]]]
    out = [pc + 1] if pc + 1 < len(ins) else []
    if op.startswith("s_cbranch"):
        out.append(labels[args.split()[-1].strip()])
    return out


def _walk(ins, labels, start, region):
    """every (pc, registers of the descriptor in flight) reachable from `start` inside `region`; the registers are () when none is in flight"""
    seen, work = set(), [(start, ())]
    while work:
        pc, fl = work.pop()
        if (pc, fl) in seen or pc not in region:
            continue
        seen.add((pc, fl))
        op, args = ins[pc]
        assert op not in ("s_setpc_b64", "s_swappc_b64"), "call or indirect jump in the worker code"
        nxt = fl
        if op == FETCH:
            nxt = tuple(sorted(_sregs(args.split(",")[0])))
        elif op == "s_waitcnt" and _waits_all_lgkm(args):
            nxt = ()
        work.extend((nx, nxt) for nx in _succ(ins, labels, pc))
    return seen


def test_next_descriptor_is_in_flight_during_the_whole_arithmetic(worker):
    ins, labels, first, region = worker
    states = _walk(ins, labels, first, region)
    reach = sorted({pc for pc, _ in states})
    ops = [ins[pc][0] for pc in reach]
    # the code as built: the first task's descriptor + one hand-placed fetch in each of the two unrolled task bodies; per body four horizontal
    # passes of four dot products and three vertical passes of two packs (rows 0 / 1, then the second row from three or from four source rows)
    assert ops.count(FETCH) == 3, ops.count(FETCH)
    assert ops.count("v_dot2_u32_u16") == 32, ops.count("v_dot2_u32_u16")
    assert ops.count("v_ashr_pk_u8_i32") == 12, ops.count("v_ashr_pk_u8_i32")
    assert ops.count("s_barrier") == 2   # the barrier loop behind each task body
    for pc, fl in states:
        op, args = ins[pc]
        if op in ("v_dot2_u32_u16", "v_ashr_pk_u8_i32"):
            assert fl, f"no descriptor in flight at instruction {pc}: {op} {args}"


def test_nothing_touches_a_descriptor_in_flight(worker):
    ins, labels, first, region = worker
    n = 0
    for pc, fl in _walk(ins, labels, first, region):
        op, args = ins[pc]
        if not fl or (op == FETCH and pc == first):
            continue
        if op == FETCH:   # a second fetch before the first was retired would make the two sets indistinguishable for the wait
            pytest.fail(f"descriptor fetch at {pc} with another one in flight")
        hit = _sregs(args) & set(fl)
        assert not hit, f"instruction {pc} ({op} {args}) touches s{sorted(hit)} of a descriptor in flight"
        n += 1
    assert n > 200   # the walk did cover the two task bodies with a descriptor in flight


def test_worker_code_has_no_vector_global_load(worker):
    ins, labels, first, region = worker
    reach = {pc for pc, _ in _walk(ins, labels, first, region)}
    loads = [(pc, ins[pc]) for pc in sorted(reach) if _VLOAD.match(ins[pc][0])]
    assert not loads, loads[:4]
    assert sum(1 for pc in reach if ins[pc][0].startswith("global_store")) == 8   # row + copy, two rows, two bodies
    assert any(_VLOAD.match(op) for op, _ in ins)   # the loader wave's, outside the walk: the pattern does match this kernel's loads
