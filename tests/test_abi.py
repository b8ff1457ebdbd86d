"""CPU tests of the drop-in boundary: the C-ABI library builds for gfx950, loads, exports every
symbol include/fdb_conflict_set.h declares, and refuses to run without a GPU (no CPU fallback)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fdb_conflict_set.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fdbcs_[a-z_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    from foundationdb_amd import build, conflict_set

    build.build()
    return conflict_set.load_library()


def test_library_exports_every_declared_symbol(lib):
    from foundationdb_amd.conflict_set import LIB_PATH, SIGNATURES

    names = declared_functions()
    assert len(names) >= 20
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB_PATH], text=True)
    exported = set(l.split()[-1] for l in out.splitlines() if l.strip())
    missing = [n for n in names if n not in exported]
    assert not missing, missing
    # the Python mirror binds exactly the declared surface
    assert sorted(SIGNATURES) == names


def test_code_object_targets_gfx950(lib):
    from foundationdb_amd.conflict_set import LIB_PATH

    out = subprocess.run(
        ["/opt/rocm/bin/roc-obj-ls", LIB_PATH], capture_output=True, text=True
    )
    if out.returncode == 0 and out.stdout.strip():
        assert "gfx950" in out.stdout
    else:  # fall back to scanning the bundle
        data = open(LIB_PATH, "rb").read()
        assert b"gfx950" in data


def test_no_cpu_fallback_without_device(lib):
    import torch

    from foundationdb_amd import conflict_set as C

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(C.FdbcsError) as e:
        C.ConflictSet(0)
    assert e.value.status == C.FDBCS_E_NODEVICE


def test_nothing_is_held_after_a_set_failed_without_device(lib):
    import torch

    from foundationdb_amd import conflict_set as C

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(C.FdbcsError) as e:
        C.ConflictSet(0)
    assert e.value.status == C.FDBCS_E_NODEVICE
    assert C.live_resources() == (0, 0, 0, 0)


def test_strerror(lib):
    from foundationdb_amd import conflict_set as C

    assert C.strerror(C.FDBCS_E_VERSION).startswith("version")
    assert C.strerror(0) == "ok"


def test_product_never_imports_oracle():
    """The shipped package must not reference oracle/ (checker only)."""
    pkg = os.path.join(ROOT, "foundationdb_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in txt and "from oracle" not in txt, f
                assert "liboracle" not in txt and "skiplist_baseline" not in txt, f


def build_shim_driver(out_path):
    from foundationdb_amd import build

    build.build()
    src = os.path.join(ROOT, "tests", "cpp", "shim_driver.cpp")
    subprocess.check_call(
        ["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "include"), src, "-L",
         os.path.join(ROOT, "foundationdb_amd"), "-lfdbcs", f"-Wl,-rpath,{os.path.join(ROOT, 'foundationdb_amd')}",
         "-o", out_path]
    )
    return out_path


def test_reference_shaped_cpp_shim_compiles_and_links(tmp_path):
    """include/conflict_set_shim.hpp restores the ConflictSet.h signatures over the C-ABI."""
    assert os.path.exists(build_shim_driver(str(tmp_path / "shim_driver")))
