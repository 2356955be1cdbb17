"""CPU: the C-ABI shared library loads and exports every symbol include/pcy.h declares (no compute
calls without a GPU), and the product path fails loudly without a device."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "pcy.h")).read()
    return sorted(set(re.findall(r"\b(pcy_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as g
    g.build()
    from procyon_amd import _lib
    lib = _lib.load()
    names = _declared()
    assert len(names) == 108, len(names)      # include/pcy.h: every addition moves this and DESIGN.md section 1 together
    for n in names:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, f"{n} declared in pcy.h but not bound"
    assert set(_lib.SIGNATURES) == set(names)
    assert lib.pcy_abi_version() == _lib.ABI_VERSION


def test_no_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from procyon_amd import _lib
    from procyon_amd.engine import Context
    with pytest.raises(_lib.PcyError):
        Context.get()


def test_product_never_imports_oracle():
    for dp, _, fs in os.walk(os.path.join(ROOT, "procyon_amd")):
        for f in fs:
            if f.endswith(".py"):
                s = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", s, re.M), f


def test_no_kernel_spills_registers(tmp_path):
    """The batch-1 decode kernels keep ~70 MB of weight loads in flight while they compute.  A spilled VGPR is reloaded with a scratch
    load -- a VMEM operation, and the wait in front of its first use (`s_waitcnt vmcnt(0)`: loads return in order) drains every weight
    load in flight: five spilled registers in decode_step_kernel cost 22 % of the headline (2.57 -> 3.15 ms per token, round 4).  The
    kernels sit at the 256-register limit, so the code object's own metadata is checked: no spilled VGPR, no scratch -- for them and, since
    every GEMM / GEMV / attention kernel here streams through in-flight loads the same way, for every kernel of the library."""
    import shutil
    import subprocess
    llvm = "/opt/rocm/lib/llvm/bin"
    if not (os.path.exists(f"{llvm}/llvm-objdump") and os.path.exists(f"{llvm}/llvm-readelf")):
        pytest.skip("ROCm llvm tools not found")
    import __graft_entry__ as g
    g.build()
    so = shutil.copy(os.path.join(ROOT, "procyon_amd", "libpcy.so"), tmp_path / "libpcy.so")
    subprocess.run([f"{llvm}/llvm-objdump", "--offloading", str(so)], cwd=tmp_path, check=True, capture_output=True)
    found = {}
    for f in sorted(os.listdir(tmp_path)):
        if "hipv4-amdgcn" not in f:
            continue
        notes = subprocess.run([f"{llvm}/llvm-readelf", "--notes", str(tmp_path / f)], capture_output=True, text=True).stdout
        for blk in notes.split("- .agpr_count:")[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk)
            if not name:
                continue
            found[name.group(1)] = (int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                                    int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)))
    assert len(found) > 200 and any("decode_step_kernel" in k for k in found) and any("mlp_chain_kernel" in k for k in found), len(found)
    bad = {k: v for k, v in found.items() if v != (0, 0)}
    assert not bad, bad


def test_switch_list_matches_whole_names_only(tmp_path):
    """procyon_amd/csrc/pcy_switch.h: PCY_DISABLE is a comma-separated list of names; a name must match as a whole entry
    (`decode_step` must not be switched off by `decode_stepx`, nor `attn_o` by `xattn_o` or `attn_o_extra`), wherever it stands."""
    import subprocess
    src = tmp_path / "t.cpp"
    src.write_text('#include "pcy_switch.h"\n#include <stdio.h>\nint main(int c, char** v) { for (int i = 1; i < c; ++i) printf("%d", (int)pcy_off(v[i])); return 0; }\n')
    exe = tmp_path / "t"
    subprocess.run(["g++", "-O1", "-I", os.path.join(ROOT, "procyon_amd", "csrc"), str(src), "-o", str(exe)], check=True)

    def run(env_value, *names):
        env = dict(os.environ)
        env.pop("PCY_DISABLE", None)
        if env_value is not None:
            env["PCY_DISABLE"] = env_value
        return subprocess.run([str(exe), *names], env=env, capture_output=True, text=True, check=True).stdout

    assert run(None, "attn_o", "decode_step") == "00"
    assert run("", "attn_o") == "0"
    assert run("attn_o", "attn_o", "decode_step") == "10"
    assert run("decode_step,attn_o", "attn_o", "decode_step", "decode_layer") == "110"
    assert run("decode_stepx,xattn_o,attn_o_extra", "attn_o", "decode_step") == "00"
    assert run("xattn_o,attn_o", "attn_o") == "1"          # a later whole entry still counts
    assert run("gemv_lds", "gemv_lds", "gemv_mfma4", "lds_prefetch") == "100"


def test_switch_snapshots_compare_by_value(tmp_path):
    """procyon_amd/csrc/pcy_switch.h: the decode path takes ONE snapshot of the switches per call (PcySwitches), and a captured decode step
    is keyed on it by value.  Two environments give equal snapshots exactly when they resolve to the same values -- the packed 64-bit key
    this replaces hashed PCY_AO_XMIN into six bits in which every multiple of 64 (the defaults included) gave 0."""
    import itertools
    import re
    import subprocess
    src = tmp_path / "s.cpp"
    # argv: VAR=value pairs, "--" between the two environments; prints 1 when the snapshots are equal
    src.write_text('#include "pcy_switch.h"\n#include <stdio.h>\n'
                   'static const char* vars[] = {"PCY_DISABLE", "PCY_AO_XMIN", "PCY_NB_MAX", "PCY_MB_MAX", "PCY_NB_UB", "PCY_MB_ABL", "PCY_MC_TRACE"};\n'
                   'int main(int c, char** v) {\n  PcySwitches s[2]; int k = 0;\n  for (int i = 1; i <= c; ++i) {\n'
                   '    if (i == c || !strcmp(v[i], "--")) { s[k++] = pcy_read_switches(); for (const char* n : vars) unsetenv(n); continue; }\n'
                   '    char* eq = strchr(v[i], \'=\'); *eq = 0; setenv(v[i], eq + 1, 1);\n  }\n'
                   '  printf("%d", (int)(s[0] == s[1] && !(s[0] != s[1]) && !memcmp(&s[0], &s[1], sizeof(PcySwitches))));\n  return 0;\n}\n')
    exe = tmp_path / "s"
    subprocess.run(["g++", "-O1", "-I", os.path.join(ROOT, "procyon_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("PCY_")}

    def equal(a, b):
        """a, b: dict VAR -> value (a missing name is unset)"""
        args = [f"{k}={v}" for k, v in a.items()] + ["--"] + [f"{k}={v}" for k, v in b.items()]
        return subprocess.run([str(exe), *args], env=clean, capture_output=True, text=True, check=True).stdout == "1"

    def pairwise_different(var, values):
        for x, y in itertools.combinations(values, 2):
            assert not equal({} if x is None else {var: x}, {} if y is None else {var: y}), (var, x, y)

    assert equal({}, {})
    # unset differs from 768 through the defaults for 2 rows (1536) and 3+ rows (4096)
    pairwise_different("PCY_AO_XMIN", [None, "0", "384", "512", "768", "1024", "1536", "4096"])
    pairwise_different("PCY_NB_MAX", ["2", "6", "7", "8"])
    assert equal({}, {"PCY_NB_MAX": "6"})
    pairwise_different("PCY_MB_MAX", ["0", "9", "32"])
    assert equal({"PCY_MB_MAX": "40"}, {"PCY_MB_MAX": "32"}) and equal({"PCY_MB_MAX": "-1"}, {"PCY_MB_MAX": "0"}) and equal({}, {"PCY_MB_MAX": "0"})
    for var in ("PCY_NB_UB", "PCY_MB_ABL", "PCY_MC_TRACE"):
        assert not equal({}, {var: "1"}), var
    assert equal({}, {"PCY_NB_UB": "2"})
    # the table of PCY_DISABLE names, read from the header: the names the library and the Python side use are all in it
    text = open(os.path.join(ROOT, "procyon_amd", "csrc", "pcy_switch.h")).read()
    table = text[text.index("#define PCY_SWITCH_NAMES"):text.index("enum PcySwitch")]
    names = re.findall(r"X\((\w+)\)", table)
    assert len(names) == len(set(names)) >= 21 and {"attn_o", "decode_step", "gemv_lds", "gemv_mfma4", "finish_norm", "decode_nb", "beam_graph"} <= set(names)
    pairwise_different("PCY_DISABLE", [None] + names)
    assert equal({"PCY_DISABLE": "attn_o,gemv_lds"}, {"PCY_DISABLE": "gemv_lds,attn_o"})
    assert equal({"PCY_DISABLE": "decode_stepx"}, {}) and equal({"PCY_DISABLE": ""}, {})
    assert not equal({"PCY_DISABLE": "decode_stepx,decode_step"}, {})
