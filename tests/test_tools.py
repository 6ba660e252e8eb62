"""tools/ holds GPU-box diagnostics; this keeps them from rotting: every script must at least parse, and the ones the documents name must exist."""
import glob
import os
import py_compile
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_tool_parses():
    py = sorted(glob.glob(os.path.join(ROOT, "tools", "*.py")))
    sh = sorted(glob.glob(os.path.join(ROOT, "tools", "*.sh")))
    assert py and sh
    for f in py:
        py_compile.compile(f, doraise=True)
    for f in sh:
        assert subprocess.run(["bash", "-n", f]).returncode == 0, f


def test_tools_named_in_the_documents_exist():
    text = open(os.path.join(ROOT, "DESIGN.md")).read() + open(os.path.join(ROOT, "tools", "README.md")).read()
    for name in set(re.findall(r"tools/([A-Za-z0-9_]+\.(?:py|sh))", text)):
        assert os.path.exists(os.path.join(ROOT, "tools", name)), name


import pytest


@pytest.mark.gpu
def test_first_multi_device_command_dry_run_on_one_gpu(tmp_path):
    """tools/first_8gpu.sh, the ONE command for the first run on more than one device, as a dry run on the one test GPU (--stand-in: every rank on device 0, the
    shared-memory stand-in behind the nccl* calls; --quick: cfg4 only, 2 steps): both exchange paths at world 4, the curve's bench lines, `ppo_cpp_hip --ranks 4`, and
    the one JSON it writes -- so that the day a node exists the command is known to run."""
    import json
    from tests.test_dp_two_ranks import build_fake_rccl
    fake = build_fake_rccl(str(tmp_path))
    out = os.path.join(str(tmp_path), "first.json")
    p = subprocess.run(["bash", os.path.join(ROOT, "tools", "first_8gpu.sh"), "--out", out, "--max-gpus", "4", "--quick", "--stand-in", fake],
                       capture_output=True, text=True, timeout=1500)
    rep = json.load(open(out))
    assert p.returncode == 0, json.dumps([{k: s[k] for k in ("what", "rc", "stderr_tail")} for s in rep["steps"] if s["rc"] != 0])[:3000]
    assert rep["rccl_nranks"] == 4 and rep["distinct_devices"] == 1 and rep["replicas_bit_identical"] is True and rep["cpp_driver_replicas_byte_identical"] is True
    assert rep["peer_path_used"] is True
    assert set(rep["values"]["cfg4/rccl"]) == {"2", "4"} and set(rep["values"]["cfg4/single"]) == {"1"} and all(v > 0 for v in rep["values"]["cfg4/auto"].values())


def test_the_pytest_tail_carries_the_finding_of_a_failed_and_an_xfailed_test(tmp_path):
    """tests/conftest.py's terminal summary: one line per failed / xfailed test with the head of its assertion message, at the very END of the output (`pytest -q` prints nothing
    for an xfail, and round 5's finding was lost in exactly that way).  A throw-away test file run under this repository's conftest."""
    import sys
    import shutil
    d = tmp_path / "tests"
    d.mkdir()
    shutil.copy(os.path.join(ROOT, "tests", "conftest.py"), str(d / "conftest.py"))
    (d / "test_x.py").write_text(
        "import pytest\n"
        "def test_plain():\n    assert 1 + 1 == 3, 'first differing buffer: thetaT'\n"
        "@pytest.mark.xfail(strict=False, reason='open')\n"
        "def test_expected():\n    raise AssertionError('handle 1 differs first at iteration 1: loss rows')\n")
    p = subprocess.run([sys.executable, "-m", "pytest", str(d), "-q", "-p", "no:cacheprovider"], capture_output=True, text=True, cwd=str(tmp_path))
    tail = p.stdout.strip().splitlines()[-12:]
    text = "\n".join(tail)
    assert "findings (tests/conftest.py)" in text
    assert any(l.startswith("FAILED") and "first differing buffer: thetaT" in l for l in tail), text
    assert any(l.startswith("XFAILED") and "handle 1 differs first at iteration 1: loss rows" in l for l in tail), text


def _listing(kernels):
    """A made-up device listing in the compiler's layout: {name: (body lines, vgpr_count)}."""
    out = ["\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"", "\t.text"]
    for i, (name, (body, _)) in enumerate(kernels.items()):
        out += ["\t.globl\t%s" % name, "\t.type\t%s,@function" % name, "%s:    ; @%s" % (name, name), "; %bb.0:"] + body
        out += ["\t.section\t.rodata,\"a\",@progbits", "\t.amdhsa_kernel %s" % name, "\t\t.amdhsa_next_free_vgpr 8", "\t.end_amdhsa_kernel", "\t.text",
                ".Lfunc_end%d:" % i, "\t.size\t%s, .Lfunc_end%d-%s" % (name, i, name)]
    out += ["\t.amdgpu_metadata", "---", "amdhsa.kernels:"]
    for name, (_, vgpr) in kernels.items():
        out += ["  - .agpr_count:     0", "    .args:", "      - .offset:         0", "        .size:           8", "    .group_segment_fixed_size: 0",
                "    .kernarg_segment_size: 8", "    .name:           %s" % name, "    .private_segment_fixed_size: 0", "    .sgpr_count:     10",
                "    .sgpr_spill_count: 0", "    .symbol:         %s.kd" % name, "    .vgpr_count:     %d" % vgpr, "    .vgpr_spill_count: 0"]
    out += ["amdhsa.target:   amdgcn-amd-amdhsa--gfx950", "...", "\t.end_amdgpu_metadata"]
    return "\n".join(out) + "\n"


def _body(bb, comment="", swap=False):
    ins = ["\tv_add_f32_e32 v1, v0, v0", "\tv_mul_f32_e32 v2, v1, v1"]
    return ["\ts_load_dwordx2 s[0:1], s[4:5], 0x0", "\ts_cbranch_scc1 .LBB%d_2%s" % (bb, comment), "; %bb.1:"] + ins[::-1 if swap else 1] + \
           [".LBB%d_2:%s" % (bb, comment), "\ts_endpgm"]


def test_kernel_code_diff_on_made_up_listings():
    """tools/kernel_code_diff.py: label numbers and comments do not count; a swapped instruction, a missing kernel and a changed metadata figure are each reported."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("kernel_code_diff", os.path.join(ROOT, "tools", "kernel_code_diff.py"))
    kcd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kcd)
    base = kcd.parse(_listing({"_Z3fooPf": (_body(0), 8), "_Z3barPf": (_body(1), 8)}))
    assert set(base) == {"_Z3fooPf", "_Z3barPf"} and len(base["_Z3fooPf"][0]) == 6 and base["_Z3fooPf"][1]["vgpr_count"] == 8

    def diff(kernels):
        rep = kcd.compare(base, kcd.parse(_listing(kernels)))
        return rep, kcd.report(rep, len(base), len(kernels))
    # the same code behind other label numbers (another kernel order) and other comments
    rep, text = diff({"_Z3barPf": (_body(0, " ; =>This Inner Loop Header"), 8), "_Z3fooPf": (_body(1), 8)})
    assert rep["same"] == 2 and not (rep["only_a"] or rep["only_b"] or rep["code"] or rep["meta"]), text
    rep, text = diff({"_Z3fooPf": (_body(0, swap=True), 8), "_Z3barPf": (_body(1), 8)})
    assert list(rep["code"]) == ["_Z3fooPf"] and rep["same"] == 1 and not rep["meta"], text
    d = rep["code"]["_Z3fooPf"]
    assert d["instructions"] == (5, 5) and d["same_opcodes"] and d["removed"] == d["added"] == 1 and "code differs: foo" in text, text
    rep, text = diff({"_Z3fooPf": (_body(0), 8)})
    assert rep["only_a"] == ["_Z3barPf"] and not rep["only_b"] and rep["same"] == 1 and "only in A: bar" in text, text
    rep, text = diff({"_Z3fooPf": (_body(0), 8), "_Z3barPf": (_body(1), 12)})
    assert rep["meta"] == {"_Z3barPf": {"vgpr_count": (8, 12)}} and not rep["code"] and rep["same"] == 1, text
