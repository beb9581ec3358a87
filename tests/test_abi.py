"""The C-ABI boundary (include/ofdm_hip.h) on CPU: the library loads, exports every
declared symbol, and rejects bad descriptors with the reference's messages before
touching the GPU."""

import ctypes
import os
import re

import numpy as np
import pytest
from conftest import ROOT

from ofdm_based_systems import _backend as B

HEADER = os.path.join(ROOT, "include", "ofdm_hip.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ofdm_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    lib = B.load_library()
    names = declared_functions()
    assert len(names) >= 18
    for n in names:
        assert hasattr(lib, n), n
        assert n in B.SIGNATURES, f"{n} has no ctypes signature"
    assert set(B.SIGNATURES) == set(names)


def test_abi_version():
    assert B.load_library().ofdm_abi_version() == B.ABI_VERSION


def _create(**kw):
    lib = B.load_library()
    d = B.Desc()
    d.n_fft = kw.get("n_fft", 64)
    d.cp = kw.get("cp", 0)
    d.prefix = kw.get("prefix", 0)
    d.precision = kw.get("precision", 1)
    d.equalizer = kw.get("equalizer", 0)
    d.n_luts = kw.get("n_luts", 0)
    d.n_taps = kw.get("n_taps", 0)
    h = ctypes.c_void_p()
    rc = lib.ofdm_plan_create(ctypes.byref(h), ctypes.byref(d), None)
    return rc, lib.ofdm_last_error().decode()


@pytest.mark.parametrize("kw,msg", [
    ({"n_fft": 3}, "power of two"),
    ({"n_fft": 8192}, "power of two"),
    ({"n_fft": 0}, "power of two"),
    ({"cp": -1}, "Prefix length must be a non-negative integer."),
    ({"n_fft": 8, "cp": 9}, "Input symbols length must be greater than prefix length."),
    ({"precision": 7}, "precision"),
    ({"equalizer": 5}, "equalizer"),
    ({"n_taps": 40}, "n_taps"),
    ({"prefix": 3}, "prefix"),
])
def test_invalid_descriptors_fail_before_the_gpu(kw, msg):
    rc, err = _create(**kw)
    assert rc == -1
    assert msg in err


def test_check_maps_invalid_to_valueerror():
    _create(n_fft=3)
    with pytest.raises(ValueError, match="power of two"):
        B.check(-1)


def test_product_has_no_cpu_fallback():
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from ofdm_based_systems.constellation.models import QAMConstellationMapper

    with pytest.raises(B.BackendUnavailable):
        QAMConstellationMapper(16).decode(np.zeros(4, np.complex128))


def test_product_library_has_no_ablation_switches():
    """The timing tools' OFDM_ABLATE_TX / _RX switches (work skipping inside the kernels) are
    compiled only into -DOFDM_ABLATION=1 builds: the product library never reads them."""
    with open(B.lib_path(), "rb") as f:
        blob = f.read()
    assert b"OFDM_ABLATE" not in blob


def test_ab_only_variant_reports_kernels_it_lacks():
    """OFDM_AB_ONLY experiment builds (tools/ab.sh variants) instantiate N = 1024..4096 only.  Every
    launcher's log2 N dispatch is with_logn (ofdm_kernels_inst.hpp), the only switch on logn in csrc/,
    which falls through to kOutOfRange; such a build defines that as kNotInBuild, and the ABI's checked()
    turns it into OFDM_E_INVALID "kernel not in this build" (ValueError in Python) instead of a HIP
    "invalid argument"; a product build keeps hipErrorInvalidValue there (N is checked at plan creation,
    so it is never reached).  The launchers' verdicts (kNotInBuild, kLdsOverflow, kNoFusedForm) are values
    no HIP call can return.  Checked on the sources, with the preprocessor branches evaluated both ways."""
    csrc = os.path.join(ROOT, "ofdm-based-systems_amd", "csrc")
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc))
               if f.endswith((".hpp", ".hip", ".h"))}
    inst, launch, abi = (sources[f] for f in ("ofdm_kernels_inst.hpp", "ofdm_launch.hpp", "ofdm_abi.hip"))
    switches = {f: re.findall(r"switch \(logn\)", text) for f, text in sources.items()}
    assert {f: len(s) for f, s in switches.items() if s} == {"ofdm_kernels_inst.hpp": 1}, switches
    with_logn = inst[inst.index("static hipError_t with_logn(int logn, F f)"):]
    with_logn = with_logn[:with_logn.index("\n}\n")]
    assert re.findall(r"switch \(logn\) \{.*?default:\s*return (\w+);", with_logn, flags=re.S) == ["kOutOfRange"]
    assert "OFDM_LOGN_CASES(" in with_logn

    def branch(text, name, ab_only):
        m = re.search(r"#ifdef OFDM_AB_ONLY\n(.*?)#else\n(.*?)#endif", text[text.index(name) - 200:], flags=re.S)
        return m.group(1 if ab_only else 2)

    assert "kOutOfRange = kNotInBuild" in branch(inst, "constexpr hipError_t kOutOfRange", True)
    assert "kOutOfRange = hipErrorInvalidValue" in branch(inst, "constexpr hipError_t kOutOfRange", False)
    assert "kAbOnly = true" in branch(launch, "constexpr bool kAbOnly", True)
    assert "kAbOnly = false" in branch(launch, "constexpr bool kAbOnly", False)

    # the translation sits in checked(), guarded by kAbOnly, and nowhere else (HIPCHK serves HIP calls)
    checked = abi[abi.index("int checked(const char* who, ofdm_plan_t p, hipError_t e, const std::string& layout_extra = {}) {"):]
    checked = checked[:checked.index("\n}\n")]
    m = re.search(r"if \(kAbOnly && e == kNotInBuild\)\s*return fail\(OFDM_E_INVALID,(.*?)\);", checked, flags=re.S)
    assert m and "kernel not in this build" in m.group(1), checked
    abi_code = re.sub(r"//[^\n]*", "", abi)
    assert abi_code.count("kernel not in this build") == 1
    for name in ("kNotInBuild", "kLdsOverflow", "kNoFusedForm"):
        assert abi_code.count(name) == 1 and name in re.sub(r"//[^\n]*", "", checked), name

    # the three verdicts: pairwise distinct, inside hipError_t's range, and no enumerator of it
    values = {name: int(v) for name, v in
              re.findall(r"constexpr hipError_t (k\w+) = static_cast<hipError_t>\((\d+)\);", launch)}
    assert set(values) == {"kNotInBuild", "kLdsOverflow", "kNoFusedForm"}, values
    assert len(set(values.values())) == 3
    header = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include", "hip", "hip_runtime_api.h")
    if os.path.exists(header):
        enum = open(header).read()
        enum = re.search(r"typedef enum\s+(?:\w+\s+)?hipError_t\s*\{(.*?)\}\s*hipError_t;", enum, flags=re.S).group(1)
        taken = {int(v) for v in re.findall(r"^\s*hip(?:Success|Error\w+)\s*=\s*(\d+)\s*,", enum, flags=re.M)}
        assert {0, 1, 701, 801} <= taken and len(taken) > 50, sorted(taken)
    else:
        taken = {0, 1, 701, 801}  # hipSuccess, InvalidValue, LaunchOutOfResources, NotSupported
    # (an enum without a fixed type holds every value of the smallest bit-field that holds its
    # enumerators: the largest is below 2048)
    assert max(taken) < 2048
    for name, v in values.items():
        assert v not in taken and 0 < v < 2048, (name, v)
