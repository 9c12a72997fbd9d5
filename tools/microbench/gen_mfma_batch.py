#!/usr/bin/env python3
"""Writes tools/microbench/mfma_batch_gen.inc for mfma_batch.hip (the distance form on the idle matrix pipe).

Two versions of the 64 pair slots of one dfire_bm_pairs batch (lane = pose), same LUT / table reads / 64-bit adds:

  MB_BATCH_VALU   the product's block (lightdock-rust_amd/tools/gen_bm_batch_asm.py): E by v_pk_add_f32 + 3 v_pk_fma_f32 per two slots
  MB_BATCH_MFMA   E by v_mfma_f32_4x4x1_16b_f32: 16 blocks of 4 x 4 outer products, block = 4 lanes (= 4 poses), D_b[r][j] = A_b[r] B_b[j] + C:
                  register r of lane j = receptor atom r against lane j's OWN ligand atom -- lane = pose survives, the receptor atom is
                  an instruction constant (the cube row's address stays a constant).  A = the receptor operand of atom 4G + (lane % 4)
                  (a lane-patterned VGPR per group G and component), B = the lane's ligand component, C = the chain:
                      D = 1 * (-l2) + RsT_G        (RsT_G: four VGPRs holding Rs of the group's four atoms, broadcast)
                      D = Rz * lz + D;  D = Ry * ly + D;  D = Rx * lx + D          -- bm_cell's operations in bm_cell's order
                  4 MFMAs per 4 slots.  A stage = 2 ligand atoms x 4 receptor atoms (two chains interleaved); its E values are
                  converted ONE STAGE LATER (no MFMA -> VALU hazard inside an asm statement, where the compiler inserts no wait states).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "lightdock-rust_amd", "tools"))
import gen_bm_batch_asm as prod  # noqa: E402

ROW = 176
D0 = 204          # v[204:219]: two sets of 8 E values (stage parity)
TS = 220          # v[220:235]: table values
CS = 236          # v[236:251]: cells / codes, two sets of 8


# r08 (the batch schedule at two waves per SIMD): (macro tag, description, prod.schedule arguments)
SCHEDULES = [
    ("BASE", "8 stages of 8 again, from schedule()", dict()),
    ("A", "(a) four E chains", dict(chains=4)),
    ("B", "(b) LUT reads two stages ahead", dict(dl=2)),
    ("C", "(c) two sets of table values", dict(dt=2)),
    ("D", "(d) ligand-half-major order", dict(half_major=True)),
    ("AC", "(a)+(c)", dict(chains=4, dt=2)),
    ("BC", "(b)+(c)", dict(dl=2, dt=2)),
    ("ABC", "(a)+(b)+(c)", dict(chains=4, dl=2, dt=2)),
    ("ACD", "(a)+(c)+(d)", dict(chains=4, dt=2, half_major=True)),
    ("G4_11", "granules of 4 slots, distances 1/1", dict(G=4)),
    ("G4_12", "granules of 4 slots, distances 1/2", dict(G=4, dt=2)),
    ("G4_22", "granules of 4 slots, distances 2/2", dict(G=4, dl=2, dt=2)),
    ("G4_23", "granules of 4 slots, distances 2/3", dict(G=4, dl=2, dt=3)),
    ("G4_33", "granules of 4 slots, distances 3/3", dict(G=4, dl=3, dt=3)),
    ("G4_13", "granules of 4 slots, distances 1/3", dict(G=4, dt=3)),
    ("S4_21", "granules of 4, reads spread, distances 2/1", dict(G=4, dl=2, dt=1, spread=True)),
    ("S4_22", "granules of 4, reads spread, distances 2/2", dict(G=4, dl=2, dt=2, spread=True)),
    ("S4_23", "granules of 4, reads spread, distances 2/3", dict(G=4, dl=2, dt=3, spread=True)),
    ("S4_32", "granules of 4, reads spread, distances 3/2", dict(G=4, dl=3, dt=2, spread=True)),
    ("S4_33", "granules of 4, reads spread, distances 3/3", dict(G=4, dl=3, dt=3, spread=True)),
    ("S4_42", "granules of 4, reads spread, distances 4/2", dict(G=4, dl=4, dt=2, spread=True)),
    ("G4_23D", "granules of 4 slots, 2/3, (d)", dict(G=4, dl=2, dt=3, half_major=True)),
]
NOLDS_TOO = ("A",)


def rows_of(h):
    """slot k of stage h -> (ligand atom i, receptor atom j): ligand atoms 2 (h % 4) + (k / 4), receptor atoms 4 (h / 4) + k % 4"""
    return [((2 * (h % 4) + k // 4), 4 * (h // 4) + k % 4) for k in range(8)]


def stage_m(h):
    G, d = h // 4, D0 + 8 * (h % 2)
    out = []
    for step in range(4):
        for t in range(2):
            i = 2 * (h % 4) + t
            dst = "v[%d:%d]" % (d + 4 * t, d + 4 * t + 3)
            if step == 0:
                out.append("v_mfma_f32_4x4x1_16b_f32 %s, %%[ones], %%[nl2_%d], %%[rst%d]" % (dst, i, G))
            else:
                c = "zyx"[step - 1]
                out.append("v_mfma_f32_4x4x1_16b_f32 %s, %%[a%s%d], %%[l%s_%d], %s" % (dst, c, G, c, i, dst))
    return out


def stage_a(h):
    d, cs = D0 + 8 * (h % 2), CS + 8 * (h % 2)
    out = ["v_cvt_u32_f32 v%d, v%d" % (cs + k, d + k) for k in range(8)]
    out += ["ds_read_u8 v%d, v%d" % (cs + k, cs + k) for k in range(8)]
    return out


def stage_b(h):
    cs = CS + 8 * (h % 2)
    out = []
    for k, (i, j) in enumerate(rows_of(h)):
        out.append("ds_read_b64 v[%d:%d], v%d offset:%%c[cube]+%d" % (TS + 2 * k, TS + 2 * k + 1, cs + k, (i * 8 + j) * ROW))
    return out


def stage_c(h):
    out = []
    for k in range(8):
        acc = "%[acc]" if k % 2 == 0 else "%[acc1]"
        out.append("v_lshl_add_u64 %s, v[%d:%d], 0, %s" % (acc, TS + 2 * k, TS + 2 * k + 1, acc))
    return out


def mfma_lines(valu_only=False, mfma_only=False):
    lines = []
    for h in range(11):
        if h < 8 and not valu_only:
            lines += stage_m(h)
        if mfma_only:
            continue
        if 1 <= h <= 8:
            lines += stage_a(h - 1)
        if h >= 2:
            lines.append("s_waitcnt lgkmcnt(%d)" % (8 if h <= 8 else 0))
        if h >= 3:
            lines += stage_c(h - 3)
        if 2 <= h <= 9:
            lines += stage_b(h - 2)
    return lines


def write_macro(f, name, lines, outs, ins, clobbers):
    f.write("// %s: %d instructions: %d vector (%d of them MFMA), %d LDS, %d waits\n" % (
        name, len(lines), sum(l.startswith("v_") for l in lines), sum(l.startswith("v_mfma") for l in lines),
        sum(l.startswith("ds_") for l in lines), sum(l.startswith("s_waitcnt") for l in lines)))
    f.write("#define %s \\\n  asm volatile( \\\n" % name)
    f.write(" \\\n".join('    "%s\\n\\t"' % l for l in lines) + " \\\n")
    f.write("    : " + ", ".join(outs) + " \\\n    : " + ", \\\n      ".join(ins) + " \\\n    : " + ", ".join(clobbers) + ', "memory")\n\n')


def main():
    path = os.path.join(HERE, "mfma_batch_gen.inc")
    with open(path, "w") as f:
        f.write("// GENERATED by tools/microbench/gen_mfma_batch.py -- do not edit.\n")
        # the block in 8 stages of 8 slots (the product's until r07), verbatim
        lines = []
        for h in range(10):
            if h < 8:
                lines += prod.stage_a(h)
            if h >= 1:
                lines.append("s_waitcnt lgkmcnt(%d)" % (8 if h < 8 else 0))
            if h >= 2:
                lines += prod.stage_c(h - 2)
            if 1 <= h <= 8:
                lines += prod.stage_b(h - 1)
        ins = []
        for name, arr in (("rs", "Rs"), ("rz", "Rz"), ("ry", "Ry"), ("rx", "Rx")):
            ins += ['[%s%d] "s"(%s[%d])' % (name, g, arr, g) for g in range(4)]
        for name, arr in (("l2", "L2"), ("lz", "LZ"), ("ly", "LY"), ("lx", "LX")):
            ins += ['[%s%d] "v"(%s[%d])' % (name, p, arr, p) for p in range(4)]
        ins.append('[cube] "n"(CUBE)')
        outs = ['[acc] "+v"(acc0)', '[acc1] "+v"(acc1)']
        write_macro(f, "MB_BATCH_VALU", lines, outs, ins, ['"v%d"' % r for r in range(220, 256)])
        # LDS sensitivity of the product's block (timing only, wrong sums): the table reads 32 bits wide; no LUT read (the cell's low
        # bits as the code); neither; and the block without any vector instruction of the distance form (cells = what the registers hold)
        b32 = [l.replace("ds_read_b64 v[%d:%d]" % (220 + 2 * k, 221 + 2 * k), "ds_read_b32 v%d" % (220 + 2 * k)) for l in lines for k in [0] if True]
        def narrow(ls):
            out = []
            for l in ls:
                if l.startswith("ds_read_b64"):
                    reg = l.split()[1].split(":")[0].replace("v[", "v")
                    l = "ds_read_b32 %s, %s" % (reg, l.split(", ", 1)[1])
                out.append(l)
            return out
        def no_lut(ls):
            return [("v_and_b32 %s, 0x78, %s" % (l.split()[1].rstrip(","), l.split()[1].rstrip(","))) if l.startswith("ds_read_u8") else l for l in ls]
        def fix_waits(ls):   # (without the LUT reads a stage's wait counts only the table reads)
            return [l.replace("lgkmcnt(8)", "lgkmcnt(0)") for l in ls]
        write_macro(f, "MB_BATCH_VALU_B32", narrow(lines), outs, ins, ['"v%d"' % r for r in range(220, 256)])
        write_macro(f, "MB_BATCH_VALU_NOLUT", fix_waits(no_lut(lines)), outs, ins, ['"v%d"' % r for r in range(220, 256)])
        write_macro(f, "MB_BATCH_VALU_NOLUT_B32", fix_waits(no_lut(narrow(lines))), outs, ins, ['"v%d"' % r for r in range(220, 256)])
        write_macro(f, "MB_BATCH_VALU_NOLDS", [l for l in fix_waits(no_lut(lines)) if not l.startswith("ds_read_b64")], outs, ins, ['"v%d"' % r for r in range(220, 256)])
        # the product's block with its 36 temporaries at v132..v167: what a kernel of 168 registers -- THREE waves per SIMD -- would run
        prod.T0 = 132
        lines3 = []
        for h in range(10):
            if h < 8:
                lines3 += prod.stage_a(h)
            if h >= 1:
                lines3.append("s_waitcnt lgkmcnt(%d)" % (8 if h < 8 else 0))
            if h >= 2:
                lines3 += prod.stage_c(h - 2)
            if 1 <= h <= 8:
                lines3 += prod.stage_b(h - 1)
        prod.T0 = 220
        write_macro(f, "MB_BATCH_VALU_T132", lines3, outs, ins, ['"v%d"' % r for r in range(132, 168)])
        # the MFMA form and its two halves (what each pipe costs alone)
        mins = ['[ones] "v"(ONES)']
        mins += ['[rst%d] "v"(RsT[%d])' % (g, g) for g in range(2)]
        for c in "zyx":
            mins += ['[a%s%d] "v"(A%s[%d])' % (c, g, c.upper(), g) for g in range(2)]
        for i in range(8):
            mins += ['[nl2_%d] "v"(NL2[%d])' % (i, i)] + ['[l%s_%d] "v"(L%s1[%d])' % (c, i, c.upper(), i) for c in "zyx"]
        mins.append('[cube] "n"(CUBE)')
        clob = ['"v%d"' % r for r in range(D0, 252)]
        write_macro(f, "MB_BATCH_MFMA", mfma_lines(), outs, mins, clob)
        # r08: schedules of the product's 64 slots (prod.schedule: granule, LUT -> table and table -> add distances, E chains, quad
        # order); the same slots, rows and sums as MB_BATCH_VALU -- the host compares every form's sums with its.  "_NOLDS": timing only.
        forms = []
        for tag, text, kw in SCHEDULES:
            sl, t0 = prod.schedule(**kw)
            clob_s = ['"v%d"' % r for r in range(t0, 256)]
            write_macro(f, "MB_S_" + tag, sl, outs, ins, clob_s)
            forms.append((len(forms) + 10, "MB_S_" + tag, "%s [%d regs]" % (text, 256 - t0), 1))
            if tag in NOLDS_TOO:
                write_macro(f, "MB_S_%s_NOLDS" % tag, [l for l in fix_waits(no_lut(sl)) if not l.startswith("ds_read_b64")], outs, ins, clob_s)
                forms.append((len(forms) + 10, "MB_S_%s_NOLDS" % tag, text + ", no LDS read at all", 0))
        f.write("// X(form number, macro, description, sums comparable with the product's)\n#define MB_SCHED_FORMS(X) \\\n")
        f.write(" \\\n".join('    X(%d, %s, "%s", %d)' % fm for fm in forms) + "\n")
        write_macro(f, "MB_BATCH_MFMA_ONLY", mfma_lines(mfma_only=True), outs, mins, clob)
        write_macro(f, "MB_BATCH_REST_ONLY", mfma_lines(valu_only=True), outs, mins, clob)
    print("wrote", path)


if __name__ == "__main__":
    main()
