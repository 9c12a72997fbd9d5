"""The rigid culling kernel reads its receptor boxes from LDS as whole 16-byte pieces.

A box is 32 bytes with a spare last word; left to itself the compiler narrows the read of its second half to `ds_read_b96`, which
the LDS serves in 8 groups of 8 lanes on 32 banks -- 8 cycles, 16 with the boxes' 32-byte stride -- where `ds_read_b128` takes 4:
a step of the loop over the surviving tiles then costs 20 LDS cycles instead of 8, and the kernel 12 % more time.  The kernel keeps
the spare words alive in empty `asm` statements; nothing in its results depends on that, so only the built code can show that
it still holds: the gfx950 code object of the library is disassembled and `dfire_bm_cull<false, false>` must hold no
`ds_read_b96`, and the two `ds_read_b128` of a box (offsets 0 and 16) for each of the eight unrolled poses' steps."""
import os
import re
import struct
import subprocess

MANGLED = "dfire_bm_cullILb0ELb0"          # <COUNT = false, ANM = false>
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _code_objects(blob):
    """Every gfx950 code object of a .hip_fatbin section: a run of uncompressed offload bundles, one per translation unit."""
    at = blob.find(MAGIC)
    while at >= 0:
        n, = struct.unpack_from("<Q", blob, at + len(MAGIC))
        q = at + len(MAGIC) + 8
        for _ in range(n):
            offset, size, triple_len = struct.unpack_from("<QQQ", blob, q)
            triple = blob[q + 24:q + 24 + triple_len]
            q += 24 + triple_len
            if b"gfx950" in triple and size:
                yield blob[at + offset:at + offset + size]
        at = blob.find(MAGIC, at + len(MAGIC))


def test_rigid_culling_kernel_reads_boxes_as_whole_16_byte_pieces(pkg, tmp_path):
    fat = str(tmp_path / "fatbin")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", pkg.LIB_PATH, fat], check=True)
    objects = [o for o in _code_objects(open(fat, "rb").read()) if MANGLED.encode() in o]
    assert len(objects) == 1, "the code object that holds dfire_bm_cull<false, false>"
    elf = str(tmp_path / "dfire_bm.co")
    with open(elf, "wb") as f:
        f.write(objects[0])
    symbols = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-t", elf], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in symbols.splitlines() if MANGLED in line and " F " in line}
    assert len(names) == 1, names
    text = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--disassemble-symbols=" + names.pop(), elf],
                          check=True, capture_output=True, text=True).stdout
    reads = re.findall(r"\b(ds_read_b\d+)\b([^\n/;]*)", text)
    assert reads, "no disassembly"
    narrow = [r for r in reads if r[0] == "ds_read_b96"]
    assert not narrow, "a box read was narrowed to ds_read_b96: %d of them" % len(narrow)
    second_halves = [r for r in reads if r[0] == "ds_read_b128" and "offset:16" in r[1]]
    # per unrolled pose: the first surviving tile's box and the two alternating register sets of the step loop
    assert len(second_halves) >= 8 * 3, len(second_halves)
