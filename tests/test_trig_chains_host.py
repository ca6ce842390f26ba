"""The spelled-out polynomial steps of csrc/ilqg_trig.hpp on the host (no GPU needed)."""
import os
import subprocess


def test_spelled_out_trig_polynomials_are_the_default_form_bit_for_bit(tmp_path):
    """The rollout's step loop takes the double sine / cosine polynomials as one block of fused multiply-adds
    (trig_poly_chains: three-operand instructions on the device, __builtin_fma on the host).  tests/host/trig_chains_check.cpp
    compiles both forms for the host (plain g++ against the HIP headers) and compares sine, cosine and tangent over the
    fast-path range, dense around the multiples of pi/2: every result must be the default form's bit for bit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "trig_chains_check")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           os.path.join(root, "tests", "host", "trig_chains_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "chains:" in out.stdout and " 0 differ" in out.stdout
