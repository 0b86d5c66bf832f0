"""Where the kernels live: csrc/sots_kernels.hip is host code only, and every family header under
csrc/kernels/ compiles on its own, so its #include lines are a statement the compiler has checked.  No GPU: hipcc
cross-compiles for gfx950, syntax only."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "survival_of_the_synthesis-gpu_accelerated_frequency_modulation_parameter_matcher_amd")


def test_the_translation_unit_holds_host_code_only():
    with open(os.path.join(PKG, "csrc", "sots_kernels.hip")) as f:
        text = f.read()
    for word in ("__global__", "__device__", "__shared__"):
        assert word not in text, f"{word} in sots_kernels.hip: device code belongs in a family header under csrc/kernels/"


def test_every_family_header_compiles_alone():
    # as the shipped build sees them, and as a stamp build does (the stamp macros are empty in the first, code in the second)
    for extra in ([], ["EXTRA=-DSOTS_STAMP"]):
        out = subprocess.run(["make", "-C", PKG, "check-headers"] + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, f"make check-headers {' '.join(extra)}\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}"
