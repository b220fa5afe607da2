"""The code the compiler makes of the XCD-local step pipeline (csrc/mlp/xstep.hip): the unit holds exactly the seven
kernels its launcher names, none of them spills to scratch, and -- under the compiler the fixture was recorded with --
each kernel's VGPR count, LDS bytes and instruction count are those of tests/fixtures/xstep_codegen.json.  The
production body's schedule is fragile (HK = 7 keeps three no-op tests for 0.25 us per step), so a change that moves
it shows here before anyone measures it; re-record the fixture (python tests/test_xstep_codegen.py) together with a
timing under profiles/.  CPU only: one device-only compile to assembly, of which the kernel metadata is read and
the lines counted."""
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from cme213_sp18_amd import _build  # noqa: E402

FIXTURE = ROOT / "tests" / "fixtures" / "xstep_codegen.json"

pytestmark = pytest.mark.skipif(not os.access(_build.HIPCC, os.X_OK), reason="no hipcc")


def _compiler_version():
    out = subprocess.run([_build.HIPCC, "--version"], check=True, capture_output=True, text=True).stdout
    return next(line.strip() for line in out.splitlines() if "clang version" in line)


def _form(name):
    """xstep_kernel<DIAG, HK, RM, PIX>'s arguments out of the mangled name (...ILb<D>ELi<HK>ELi<RM>ELi<PIX>EE...)."""
    d, hk, rm, pix = map(int, re.search(r"ILb(\d)ELi(\d+)ELi(\d+)ELi(\d+)EE", name).groups())
    return f"diag{d}_hk{hk}_rm{rm}_pix{pix}"


def codegen(out_dir):
    """{form: {scratch, vgprs, lds_bytes, instructions}} of every xstep_kernel in the unit."""
    asm = Path(out_dir) / "xstep.s"
    cmd = _build._hip_compile_cmd(_build.CSRC / "mlp" / "xstep.hip", asm)
    cmd[cmd.index("-c")] = "-S"
    subprocess.run(cmd + ["--cuda-device-only"], check=True)
    text = asm.read_text()
    kernels = {}
    for m in re.finditer(r"^    \.name: +(\S*xstep_kernel\S*)$", text, re.M):
        # the kernel's metadata map: from the "- .agpr_count" that opens it to the next one (or the end of the list)
        beg = text.rfind("\n  - .", 0, m.start())
        end = text.find("\n  - .", m.end())
        meta = text[beg:end if end > 0 else len(text)]

        def field(key):
            return int(re.search(rf"^    \.{key}: +(\d+)$", meta, re.M).group(1))

        name = m.group(1)
        beg = text.index(f"\n{name}:")
        body = text[beg:text.index("\n.Lfunc_end", beg)]
        # instructions: the function's indented lines that are neither directives nor comments
        ins = sum(1 for line in body.splitlines() if line.startswith("\t") and line[1:2] not in (".", ";", ""))
        kernels[_form(name)] = {"scratch": field("private_segment_fixed_size"), "vgprs": field("vgpr_count"),
                                "lds_bytes": field("group_segment_fixed_size"), "instructions": ins}
    return kernels


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    return codegen(tmp_path_factory.mktemp("xstep_codegen"))


def test_the_unit_holds_the_seven_pipeline_kernels_without_scratch(kernels):
    assert sorted(kernels) == sorted(["diag0_hk7_rm1_pix0", "diag0_hk7_rm4_pix0", "diag0_hk7_rm3_pix0",
                                      "diag0_hk7_rm0_pix1", "diag0_hk7_rm0_pix0",
                                      "diag1_hk0_rm0_pix1", "diag1_hk0_rm0_pix0"])
    assert {k: v["scratch"] for k, v in kernels.items() if v["scratch"] != 0} == {}
    # (512-thread workgroups, one per CU: 256 VGPRs is the whole budget)
    assert all(v["vgprs"] <= 256 for v in kernels.values()), kernels


def test_the_kernels_are_the_recorded_ones(kernels):
    want = json.loads(FIXTURE.read_text())
    have = _compiler_version()
    if have != want["compiler"]:
        pytest.skip(f"recorded with another compiler ({want['compiler']!r}, here {have!r}): counts not compared")
    for form, k in kernels.items():
        print(form, k)
    assert kernels == want["kernels"]


if __name__ == "__main__":  # re-record the fixture
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        rec = {"compiler": _compiler_version(), "kernels": codegen(d)}
    FIXTURE.write_text(json.dumps(rec, indent=1, sort_keys=True) + "\n")
    print(json.dumps(rec, indent=1, sort_keys=True))
