#!/usr/bin/env python3
"""Static instruction census of the kernels in a gfx950 assembly listing (hipcc ... --cuda-device-only -S):

    python tools/isa_census.py rowwise.s k_lat_bwd_g k_lat_fwd_g

prints, per kernel whose demangled name contains one of the given substrings: VALU / SALU / vector-memory / LDS
instruction counts, the classes the latent kernels' census tracks (floating-point arithmetic, v_mov, 64-bit address
arithmetic, lane moves, v_cndmask, v_log / v_exp, exec-masked regions, s_nop), and the registers, occupancy and scratch
the assembler reports for the kernel."""
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
    kernels, cur, body, done = {}, None, None, None
    meta = collections.defaultdict(dict)
    for line in open(path):
        s = line.strip()
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            cur, body, done = m.group(1), collections.Counter(), collections.Counter()
            continue
        if cur is not None:
            if s.startswith(".amdhsa_kernel"):  # the body ends at its descriptor, not at the first s_endpgm: blocks are laid out
                kernels[cur] = done             # behind it.  The s_nop / s_code_end padding at the end is not counted.
                cur = None
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
        m = re.match(r"^\s*\.amdhsa_next_free_vgpr\s+(\d+)", line)
        if m:
            meta[mk]["vgpr"] = int(m.group(1))
        m = re.match(r"^\s*\.amdhsa_accum_offset\s+(\d+)", line)
        if m:
            meta[mk]["accum_offset"] = int(m.group(1))
        m = re.match(r"^\s*\.amdhsa_next_free_sgpr\s+(\d+)", line)
        if m:
            meta[mk]["sgpr"] = int(m.group(1))
        m = re.match(r"^\s*\.amdhsa_private_segment_fixed_size\s+(\d+)", line)
        if m:
            meta[mk]["scratch"] = int(m.group(1))
    return kernels, meta


def main():
    path, pats = sys.argv[1], sys.argv[2:]
    kernels, meta = census(path)
    names = demangle(list(kernels))
    for k, c in kernels.items():
        dn = names[k]
        if pats and not any(p in dn for p in pats):
            continue
        short = re.sub(r"\(.*", "", dn).replace("void mmvae::", "")
        valu = sum(n for op, n in c.items() if op.startswith("v_"))
        salu = sum(n for op, n in c.items() if op.startswith("s_"))
        vmem = sum(n for op, n in c.items() if op.startswith(("global_", "buffer_", "flat_", "scratch_")))
        lds = sum(n for op, n in c.items() if op.startswith("ds_"))
        pick = lambda ops: sum(c[o] for o in ops)
        md = meta.get(k, {})
        vg = md.get("vgpr", 0)
        alloc = (vg + 7) // 8 * 8
        waves = min(8, 512 // alloc) if alloc else 0
        print(f"{short}")
        print(f"  VALU {valu}  SALU {salu}  VMEM {vmem}  LDS {lds}")
        print(f"  fp arithmetic {pick(FP)}  v_mov_b32 {c['v_mov_b32']}  64-bit address {pick(ADDR64)} "
              f"({', '.join(f'{o} {c[o]}' for o in ADDR64 if c[o])})")
        print(f"  lane moves {pick(LANE)} ({', '.join(f'{o} {c[o]}' for o in LANE if c[o])})  v_cndmask_b32 {c['v_cndmask_b32']}  "
              f"v_log_f32 {c['v_log_f32']}  v_exp_f32 {c['v_exp_f32']}  ds_bpermute_b32 {c['ds_bpermute_b32']}  "
              f"DPP/permlane {c['(dpp)'] + sum(n for o, n in c.items() if 'permlane' in o)}")
        print(f"  s_and_saveexec_b64 {c['s_and_saveexec_b64']}  s_cbranch_execz {c['s_cbranch_execz']}  s_nop {c['s_nop']}  "
              f"s_waitcnt {c['s_waitcnt']}")
        print(f"  VGPRs {vg} (waves per SIMD {waves})  SGPRs {md.get('sgpr', '?')}  scratch {md.get('scratch', '?')} bytes")


if __name__ == "__main__":
    main()
