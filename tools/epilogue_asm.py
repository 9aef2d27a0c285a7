"""development probe: what the fused-convolution kernels of a built library compile to behind their K loops.

    python tools/epilogue_asm.py [libmpgan_hip.so ...]

For every conv_mfma* and conv_small* kernel: static counts of global_load_dword* (the LDS-DMA copies of the K loops are
global_load_lds_*, not counted), `s_waitcnt` with vmcnt(0), s_cbranch and scratch instructions, and registers / scratch
bytes / waves per SIMD from the code object's metadata.  These counts are over the WHOLE kernel: the blocks of a kernel
are not laid out in program order (one K loop of the F16F6 kernels sits behind the epilogue), so "behind the last MFMA"
is not a property of the listing.  Two builds whose K loops are the same source differ by their epilogues.

The property that matters is counted directly.  conv_mfma*: the register-store blocks of the G8-only path are the only
users of v_permlane32_swap; `st.blk` is how many there are (one per unrolled tile row and activation path the compiler
kept apart), `st.wait` the s_waitcnt instructions with a vmcnt field inside them, from the first swap of a block to its
last store (stores count in vmcnt on gfx950, so such a wait holds a wave until its earlier stores are acknowledged).
conv_small*: `b.gld` / `b.wait` are the global loads and vmcnt(0) waits behind the last s_barrier of the listing.
Needs the LLVM tools of ROCm, no GPU."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def code_objects(lib, tmp):
    fat = os.path.join(tmp, "fat.bin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, fat], check=True)
    blob = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
    for k, a in enumerate(starts):
        part, co = os.path.join(tmp, "part%d.bin" % k), os.path.join(tmp, "dev%d.co" % k)
        with open(part, "wb") as f:
            f.write(blob[a:starts[k + 1] if k + 1 < len(starts) else len(blob)])
        subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o",
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + part, "--output=" + co], check=True)
        yield co


def demangle(names):
    """conv_x_kernel<4, 3, false> from the Itanium name (integer and bool template arguments only)"""
    out = {}
    for n in names:
        m = re.search(r"\d+(conv_[a-z0-9_]+?)I((?:L[ib]\d+E)+)E", n)
        out[n] = "%s<%s>" % (m.group(1), ", ".join(re.findall(r"L[ib](\d+)E", m.group(2)))) if m else n
    return out


def vmcnt_zero(line):
    """an s_waitcnt that waits for every outstanding vector-memory operation"""
    if "s_waitcnt" not in line or "s_waitcnt_" in line:
        return False
    m = re.search(r"vmcnt\((\d+)\)", line)
    return m is not None and int(m.group(1)) == 0


def store_blocks(lines):
    """(blocks, vmcnt waits inside them): a block runs from a v_permlane32_swap to the last global_store that follows
    within 48 instructions of the block's last swap or store; swaps further apart than that start a new block"""
    blocks, cur = [], None
    for i, l in enumerate(lines):
        if "v_permlane32_swap" in l:
            if cur is None or i - cur[1] > 48:
                cur = [i, i]
                blocks.append(cur)
            cur[1] = i
        elif "global_store" in l and cur is not None and i - cur[1] <= 48:
            cur[1] = i
    waits = sum(1 for a, b in blocks for l in lines[a:b + 1] if "s_waitcnt" in l and "vmcnt" in l)
    return len(blocks), waits


def report(lib):
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", co], capture_output=True, text=True, check=True).stdout
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
            meta = {}
            for blk in notes.split("- .agpr_count:")[1:]:
                blk = ".agpr_count:" + blk
                f = {k: v for k, v in re.findall(r"\.(agpr_count|vgpr_count|sgpr_count|private_segment_fixed_size|name):\s+(\S+)", blk)}
                if "name" in f:
                    meta[f["name"]] = f
            bodies, name = {}, None
            for line in asm.splitlines():
                m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
                if m:
                    name = m.group(1)
                    bodies[name] = []
                elif name:
                    bodies[name].append(line)
            for name, lines in bodies.items():
                if not ("conv_mfma" in name or "conv_small" in name) or name not in meta:
                    continue
                f = meta[name]
                if "conv_mfma" in name:
                    extra = store_blocks(lines)
                else:
                    last = max((i for i, l in enumerate(lines) if "s_barrier" in l), default=-1)
                    extra = (sum("global_load_dword" in l for l in lines[last + 1:]), sum(vmcnt_zero(l) for l in lines[last + 1:]))
                regs = int(f["vgpr_count"])                  # unified file: arch + acc registers
                occ = min(8, 512 // (-(-max(regs, 1) // 8) * 8))
                rows.append((name, sum("global_load_dword" in l for l in lines), sum(vmcnt_zero(l) for l in lines),
                             sum("s_cbranch" in l for l in lines), sum("\tscratch_" in l or " scratch_" in l for l in lines), regs,
                             int(f["agpr_count"]), int(f["private_segment_fixed_size"]), occ) + extra)
    names = demangle([r[0] for r in rows])
    print("%s" % lib)
    print("%-34s %6s %8s %9s %6s %5s %5s %7s %5s %15s" % ("kernel", "gloads", "vmcnt(0)", "s_cbranch", "scr.in", "vgpr", "agpr", "scratch", "waves",
                                                           "st.blk/st.wait"))
    print("%-34s %86s" % ("", "or b.gld/b.wait"))
    for r in sorted(rows, key=lambda r: names[r[0]]):
        print("%-34s %6d %8d %9d %6d %5d %5d %7d %5d %9d / %3d" % ((names[r[0]],) + r[1:]))


if __name__ == "__main__":
    from_repo = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multi-pass-gan_amd", "csrc", "libmpgan_hip.so")
    for lib in sys.argv[1:] or [from_repo]:
        report(lib)
        print()
