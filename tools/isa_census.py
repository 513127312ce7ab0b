#!/usr/bin/env python3
"""Static instruction census of the kernels in a gfx950 assembly listing (hipcc ... --cuda-device-only -S):

    python tools/isa_census.py rowwise.s k_lat_bwd_g k_lat_fwd_g

prints, per kernel whose demangled name contains one of the given substrings: VALU / SALU / vector-memory / LDS
instruction counts, the classes the latent kernels' census tracks (floating-point arithmetic, v_mov, 64-bit address
arithmetic, lane moves, v_cndmask, v_log / v_exp, exec-masked regions, s_nop), and the registers, occupancy, scratch and
static LDS the assembler reports for the kernel.  A function that is not a kernel (a noinline device function) is listed as such.

    python tools/isa_census.py --compare parent.s head.s

prints one line per function of two listings, '=' where the census is equal and both lines where it is not."""
import collections
import re
import subprocess
import sys

FP = ("v_fma_f32", "v_fmac_f32", "v_mul_f32", "v_add_f32", "v_sub_f32", "v_fmamk_f32", "v_fmaak_f32", "v_pk_fma_f32",
      "v_pk_mul_f32", "v_pk_add_f32", "v_subrev_f32", "v_max_f32", "v_min_f32")
ADDR64 = ("v_lshl_add_u64", "v_mad_u64_u32", "v_mad_i64_i32", "v_mul_lo_u32", "v_mul_hi_u32", "v_add_co_u32",
          "v_addc_co_u32", "v_lshlrev_b64", "v_ashrrev_i32")
LANE = ("v_readlane_b32", "v_writelane_b32", "v_readfirstlane_b32")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except Exception:
        return {n: n for n in names}


def census(path):
    """-> ({name: opcode counts}, {name: registers, scratch, LDS bytes, "kernel": bool}) of every function of the listing.
    A function's body ends at its .Lfunc_end / .size, a kernel's already at its descriptor (.amdhsa_kernel, which the listing
    puts before them); a plain function (a noinline device function) has no descriptor, and its registers and scratch are
    the assembler's "; NumVgprs" / "; ScratchSize" comments behind its end."""
    kernels, cur, body, done, last = {}, None, None, None, None
    meta = collections.defaultdict(dict)
    for line in open(path):
        s = line.strip()
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            cur, body, done = m.group(1), collections.Counter(), collections.Counter()
            continue
        if cur is not None:
            if s.startswith((".amdhsa_kernel", ".Lfunc_end", ".size")):  # not at the first s_endpgm: blocks are laid out behind
                kernels[cur] = done                                      # it.  The s_nop / s_code_end padding is not counted.
                last, cur = cur, None
            elif s.startswith((";", ".", "//")) or not s or s.endswith(":"):
                continue
            else:
                op = s.split()[0]
                if op.endswith("_dpp"):
                    body["(dpp)"] += 1
                op = re.sub(r"_(e32|e64|sdwa|dpp|e64_dpp)$", "", op)     # the encoding suffixes of the listing
                body[op] += 1
                if op not in ("s_nop", "s_code_end"):
                    done = body.copy()
                continue
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            mk = m.group(1)
            meta[mk]["kernel"] = True
        for key, pat in (("vgpr", "next_free_vgpr"), ("accum_offset", "accum_offset"), ("sgpr", "next_free_sgpr"),
                         ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size")):
            m = re.match(r"^\s*\.amdhsa_" + pat + r"\s+(\d+)", line)
            if m:
                meta[mk][key] = int(m.group(1))
        m = re.match(r"^; (NumVgprs|NumSgprs|ScratchSize): (\d+)", line)
        if m and last is not None and not meta[last].get("kernel"):
            meta[last][{"NumVgprs": "vgpr", "NumSgprs": "sgpr", "ScratchSize": "scratch"}[m.group(1)]] = int(m.group(2))
    return kernels, meta


def short_name(dn):
    return re.sub(r"\(.*", "", dn).replace("void mmvae::", "")


def waves_per_simd(vgpr):
    alloc = (vgpr + 7) // 8 * 8
    return min(8, 512 // alloc) if alloc else 0


def classes(c):
    return (sum(n for op, n in c.items() if op.startswith("v_")), sum(n for op, n in c.items() if op.startswith("s_")),
            sum(n for op, n in c.items() if op.startswith(("global_", "buffer_", "flat_", "scratch_"))),
            sum(n for op, n in c.items() if op.startswith("ds_")))


def compare(parent, head):
    """One line per function of the two listings: '=' where every opcode count, the registers, scratch and LDS are equal,
    else the parent's line and the head's; a function only one of them has is marked so."""
    (kp, mp), (kh, mh) = census(parent), census(head)
    names = demangle(list(dict.fromkeys(list(kp) + list(kh))))

    def row(k, c, md):
        valu, salu, vmem, lds = classes(c)
        vg = md.get("vgpr", 0)
        return (f"VALU {valu:5d} SALU {salu:5d} VMEM {vmem:4d} LDS {lds:4d} VGPR {vg:4d} SGPR {md.get('sgpr', 0):4d} "
                f"scratch {md.get('scratch', 0)} LDS bytes {md.get('lds', 0)} waves {waves_per_simd(vg)}")

    for k, dn in names.items():
        label = short_name(dn) + ("" if (mp.get(k) or mh.get(k, {})).get("kernel") else " [function]")
        if k in kp and k in kh:
            if kp[k] == kh[k] and mp.get(k) == mh.get(k):
                print(f"{label:<60} {row(k, kh[k], mh.get(k, {}))}  =")
            else:
                print(f"{label:<60} {row(k, kp[k], mp.get(k, {}))}  parent")
                print(f"{'':<60} {row(k, kh[k], mh.get(k, {}))}  head")
        else:
            side, kk, mm = ("parent only", kp, mp) if k in kp else ("head only", kh, mh)
            print(f"{label:<60} {row(k, kk[k], mm.get(k, {}))}  {side}")


def main():
    if sys.argv[1] == "--compare":
        return compare(sys.argv[2], sys.argv[3])
    path, pats = sys.argv[1], sys.argv[2:]
    kernels, meta = census(path)
    names = demangle(list(kernels))
    for k, c in kernels.items():
        dn = names[k]
        if pats and not any(p in dn for p in pats):
            continue
        valu, salu, vmem, lds = classes(c)
        pick = lambda ops: sum(c[o] for o in ops)
        md = meta.get(k, {})
        vg = md.get("vgpr", 0)
        waves = waves_per_simd(vg)
        print(short_name(dn) + ("" if md.get("kernel") else "  [a function, not a kernel]"))
        print(f"  VALU {valu}  SALU {salu}  VMEM {vmem}  LDS {lds}")
        print(f"  fp arithmetic {pick(FP)}  v_mov_b32 {c['v_mov_b32']}  64-bit address {pick(ADDR64)} "
              f"({', '.join(f'{o} {c[o]}' for o in ADDR64 if c[o])})")
        print(f"  lane moves {pick(LANE)} ({', '.join(f'{o} {c[o]}' for o in LANE if c[o])})  v_cndmask_b32 {c['v_cndmask_b32']}  "
              f"v_log_f32 {c['v_log_f32']}  v_exp_f32 {c['v_exp_f32']}  ds_bpermute_b32 {c['ds_bpermute_b32']}  "
              f"DPP/permlane {c['(dpp)'] + sum(n for o, n in c.items() if 'permlane' in o)}")
        print(f"  s_and_saveexec_b64 {c['s_and_saveexec_b64']}  s_cbranch_execz {c['s_cbranch_execz']}  s_nop {c['s_nop']}  "
              f"s_waitcnt {c['s_waitcnt']}")
        print(f"  VGPRs {vg} (waves per SIMD {waves})  SGPRs {md.get('sgpr', '?')}  scratch {md.get('scratch', '?')} bytes  "
              f"LDS {md.get('lds', 0)} bytes")


if __name__ == "__main__":
    main()
