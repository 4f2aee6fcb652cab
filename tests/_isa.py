"""Device-ISA helpers of the CPU-only kernel soundness tests (a plain helper module, not a conftest): compile a translation
unit of ml-inference-optimizer_amd/csrc to gfx950 assembly with the Makefile's flags, split it into kernels, and the two
checks the hand-scheduled kernels must pass -- no compiler-generated use of the accumulator registers their inline asm owns
(tools/check_agpr.py), and no spill within 256 VGPRs (the kernel metadata)."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ml-inference-optimizer_amd", "csrc")
# the Makefile's CXXFLAGS, and FA_FLAGS: what it adds for the attention units
CXXFLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I../../include", "-I.", "-Wno-unused-value",
            "-Wno-inline-asm"]
FA_FLAGS = ["-mllvm", "-amdgpu-mfma-vgpr-form", "-fno-slp-vectorize"]


def device_isa(tmp_path, src, defines, attention=True):
    """The file (under tmp_path) of the device assembly of csrc/<src> compiled with -D<define> for each of defines (plus
    FA_FLAGS when attention).  Skips the test when hipcc is missing."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    isa = tmp_path / (os.path.splitext(src)[0] + "".join("_" + d.replace("=", "") for d in defines) + ".s")
    cmd = [hipcc, *CXXFLAGS, *(FA_FLAGS if attention else []), *("-D" + d for d in defines), "-S", "--cuda-device-only",
           src, "-o", str(isa)]
    subprocess.run(cmd, cwd=CSRC, check=True, capture_output=True)
    return isa


def fa_isa(tmp_path, src, type_id, D) -> str:
    """The device assembly text of an attention unit for one (dtype, padded head dim)."""
    return device_isa(tmp_path, src, [f"FA_TYPE_ID={type_id}", f"FA_D={D}"]).read_text()


def kernels(text, mangled) -> list:
    """The code of every kernel whose mangled name starts with `mangled`: its lines from the label to s_endpgm."""
    lines = text.splitlines()
    starts = [i for i, l in enumerate(lines) if re.match(rf"^{mangled}\w+:", l)]
    return [lines[a:next(i for i in range(a, len(lines)) if "s_endpgm" in lines[i]) + 1] for a in starts]


def metadata(text, name_re) -> list:
    """The metadata entries of the kernels whose mangled name matches name_re."""
    return re.findall(rf"\.name:\s+{name_re}\n(?:.*\n){{0,12}}", text)


def fa3_agpr_floor(D) -> int:
    return 16 * (14 - 2 * (D // 32)) - 4 - 8 * (D // 16)  # Fa3Map<D>::A_Q


def check_agpr(tmp_path, body, floor) -> None:
    """No compiler-generated instruction of the kernel touches an accumulator register >= floor (tools/check_agpr.py),
    and nothing spills."""
    part = tmp_path / "k.s"
    part.write_text("\n".join(body))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_agpr.py"), str(part), str(floor)],
                       capture_output=True, text=True)
    assert r.returncode == 0, body[0] + "\n" + r.stdout
    assert not any("scratch_" in l for l in body), "register spills in " + body[0]


def check_fits_256(blk, no_spill=True) -> None:
    """A kernel's metadata entry: at most 256 VGPRs (two waves per SIMD), and -- if no_spill -- no scratch."""
    if no_spill:
        assert re.search(r"\.private_segment_fixed_size:\s+0\b", blk), blk
        assert re.search(r"\.vgpr_spill_count:\s+0\b", blk), blk
    assert int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)) <= 256, blk
