"""Static checks on the likelihood draws of the one-lane-per-voxel fused kernels that hold their wave-uniform operands
in vector registers (voxel_mc_sums<.., DREGS>, LikRegs, elbo_core.h / qbold_dev.h; kDrawRegs, vi_fwd_kernels.inc),
cross-compiled for gfx950 without a GPU with the fixtures of tests/test_vi_fwd_vox_listing.py.

Two stretches of a kernel's listing are read, found by landmarks in its text:

  - the likelihood draw body: behind the sampling phase's `s_setprio 1`, from the draw's `v_cvt_f32_u32_sdwa` (Box-Muller's
    radius word) to the last branch back to a label in front of it.  It runs once per likelihood draw.  The stretch
    ends behind the share loop's tail (share_sum and the loop counters, a few instructions that run once per share and
    sit behind the draw in the text), so the figure is a little more than the draw alone; it is the same stretch on
    either side of the comparison and gives the 134 the change started from.
  - the whitened KL call body: behind the `s_setprio 2` that follows, the shortest loop that holds exactly four
    `v_sin_f32` (a Philox call serves four draws).  It runs once per KL call.

In them: vector instructions (MFMAs apart), those with an SGPR among their sources, `v_mov_b32` whose source is an SGPR
or a literal, and LDS reads narrower than the 128-bit table rows.

                                       likelihood draw body                       whitened KL call body
                                       vector / moves / SGPR-source / LDS reads   vector / moves / SGPR-source
  vox_fold<11,2,2,false,1024> parent   134 / 9 / 13 / 13 (5 narrow)               73 / 2 / 30
                              tree     125 / 0 /  1 /  8 (0 narrow)               73 / 2 / 30
  vox_fold<24,2,7,false,768>  parent   224 / 19 / 23 / 31 (15 narrow)             73 / 2 / 30
                              tree     205 / 0 /  1 / 16 (0 narrow)               73 / 2 / 30
  vox<24,2,7,false,768>       parent   224 / 19 / 23 / 31 (15 narrow)             73 / 2 / 30
                              tree     205 / 0 /  1 / 16 (0 narrow)               73 / 2 / 30

The source left in the likelihood body is the exponent word of bm_angle's v_alignbit_b32.

The KL call body is printed and NOT bounded.  Registers for the whitened KL loop (Philox keys and multipliers, scalar
key mixes of the first rounds) were built, brought the call to 72 / 0 / 3, and measured 0.35 % slower on the MI355X than
the parent; they were dropped (MEASUREMENTS 34), and with them the bound of six SGPR sources per call that went with
them.  The loop is the parent's.

The classic vi_fwd_kernel_vox<11,2,2,false,1024> does not have the registers (12 bytes of scratch with them) and is the
one instance switched off: it must stay out of scratch, and its draw loops still show the SGPR operands."""
import re

import pytest

from test_vi_fwd_vox_listing import KERNELS, VGPR_BUDGET, kernel_body, listing, opcode  # noqa: F401

FOLD_KERNELS = {T: k.replace("vi_fwd_kernel_voxI", "vi_fwd_kernel_vox_foldI") for T, k in KERNELS.items()}
# the parent commit's listing under this counter: vector instructions of the likelihood draw body
PARENT_LIK_VALU = {11: 134, 24: 224}
TWO_DESTS = ("v_mad_u64_u32", "v_mad_i64_i32", "v_add_co_u32", "v_sub_co_u32", "v_subrev_co_u32", "v_addc_co_u32",
             "v_subb_co_u32", "v_subbrev_co_u32", "v_div_scale_f32", "v_div_scale_f64")
SGPR = re.compile(r"^(s\d+|s\[\d+:\d+\]|ttmp\d+)$")


def operands(line):
    t = line.split(";")[0].strip()
    parts = t.split(None, 1)
    if len(parts) < 2:
        return []
    # split on commas outside brackets
    return [o.strip() for o in re.split(r",\s*(?![^\[]*\])", parts[1])]


def sources(line):
    op = opcode(line)
    ops = operands(line)
    ops = ops[2:] if op.startswith(TWO_DESTS) else ops[1:]
    # drop modifiers that follow the operands without a comma (`v1 dst_sel:DWORD ...`) and the sign / abs wrappers
    return [o.split()[0].lstrip("-|").rstrip("|") for o in ops if o]


def is_valu(line):
    op = opcode(line)
    return bool(op) and op.startswith("v_") and not op.startswith("v_mfma")


def has_sgpr_source(line):
    return any(SGPR.match(s) for s in sources(line))


def is_uniform_move(line):
    """v_mov_b32 from an SGPR or a literal (inline constants are part of the encoding and are not literals)."""
    if opcode(line) != "v_mov_b32_e32" and opcode(line) != "v_mov_b32":
        return False
    src = sources(line)[0]
    if SGPR.match(src):
        return True
    if re.match(r"^v\d+$", src):
        return False
    if re.match(r"^0x[0-9a-fA-F]+$", src):
        return True
    if re.match(r"^-?\d+$", src):
        return not -16 <= int(src) <= 64
    return False   # 0.5, 1.0, 2.0, 4.0 and their negatives: inline


def labels_of(body):
    return {l.split(":")[0].strip(): i for i, l in enumerate(body) if re.match(r"^\.LBB\w+:", l)}


def branch_target(body, i, labels):
    op = opcode(body[i])
    if op and (op.startswith("s_cbranch") or op == "s_branch"):
        return labels.get(body[i].split(";")[0].split()[-1])
    return None


def prio_at(body, start, level):
    return next(i for i in range(start, len(body))
                if opcode(body[i]) == "s_setprio" and body[i].split(";")[0].split()[-1] == str(level))


def sampling_start(body):
    ops = [opcode(l) for l in body]
    last_mfma = max(i for i, o in enumerate(ops) if o and o.startswith("v_mfma"))
    return prio_at(body, last_mfma, 1)


def lik_draw_body(body):
    labels = labels_of(body)
    start = sampling_start(body)
    cvt = next(i for i in range(start, len(body)) if (opcode(body[i]) or "").startswith("v_cvt_f32_u32_sdwa"))
    # the last branch back in front of the KL phase: the draw's tau block sits behind an always-taken scalar branch
    # (qb_phase_fence) whose not-taken side jumps back too, so the first branch back is not the end of the draw
    end = prio_at(body, cvt, 2)
    back = [i for i in range(cvt, end) if (branch_target(body, i, labels) or len(body)) < cvt]
    assert back, "no branch back behind the likelihood draw"
    return body[cvt:back[-1] + 1]


def kl_call_body(body):
    labels = labels_of(body)
    start = prio_at(body, sampling_start(body) + 1, 2)
    end = next(i for i in range(start, len(body)) if opcode(body[i]) == "s_barrier")
    loops = []
    for i in range(start, end):
        t = branch_target(body, i, labels)
        if t is not None and start <= t < i:
            seg = body[t:i + 1]
            if sum(1 for l in seg if (opcode(l) or "").startswith("v_sin_f32")) == 4:
                loops.append(seg)
    assert loops, "no loop with four v_sin_f32 behind the KL phase's s_setprio"
    return min(loops, key=len)


def figures(seg):
    valu = [l for l in seg if is_valu(l)]
    return {
        "valu": len(valu),
        "moves": [l.strip() for l in valu if is_uniform_move(l)],
        "sgpr": [l.strip() for l in valu if has_sgpr_source(l)],
        "lds": [l.strip() for l in seg if (opcode(l) or "").startswith("ds_read")],
    }


def show(name, what, f):
    narrow = [l for l in f["lds"] if not opcode(l).startswith("ds_read_b128")]
    print(f"{name} {what}: {f['valu']} vector instructions, {len(f['moves'])} uniform moves, {len(f['sgpr'])} with an "
          f"SGPR source, {len(f['lds'])} LDS reads ({len(narrow)} narrower than 128 bits)")
    for l in f["moves"] + f["sgpr"] + narrow:
        print("    " + l)
    return narrow


# (T, kernel): the folded split-f16 kernels and the classic one at T = 24, all switched on
SWITCHED_ON = {"fold-11": (11, FOLD_KERNELS[11]), "fold-24": (24, FOLD_KERNELS[24]), "classic-24": (24, KERNELS[24])}


@pytest.mark.parametrize("which", list(SWITCHED_ON))
def test_switched_on_kernels(listing, which):
    T, name = SWITCHED_ON[which]
    body, res = kernel_body(listing, name)
    print(f"{name}: {res}")
    assert res["ScratchSize"] == 0
    assert res.get("TotalNumVgprs", res["NumVgprs"]) <= VGPR_BUDGET[T]
    lik = figures(lik_draw_body(body))
    narrow = show(name, "likelihood draw body", lik)
    assert not lik["moves"]
    assert not narrow
    assert len(lik["sgpr"]) <= 2
    if T == 11:
        assert lik["valu"] <= 126
    assert lik["valu"] < PARENT_LIK_VALU[T]
    show(name, "whitened KL call body (the parent's loop: not bounded)", figures(kl_call_body(body)))


def test_classic_kernel_stays_out_of_scratch(listing):
    body, res = kernel_body(listing, KERNELS[11])
    print(f"{KERNELS[11]}: {res}")
    show(KERNELS[11], "likelihood draw body", figures(lik_draw_body(body)))
    show(KERNELS[11], "whitened KL call body", figures(kl_call_body(body)))
    assert res["ScratchSize"] == 0
    assert res.get("TotalNumVgprs", res["NumVgprs"]) <= VGPR_BUDGET[11]
