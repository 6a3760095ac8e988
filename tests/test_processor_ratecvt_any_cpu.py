"""The fused any-length TX quantum (include/fskhip_next.h: fskhip_processor_process_ratecvt_any_*, fskhip_processor_last_tx_kernel)
without a GPU:
  * where the kernel's any-length form starts and which form a quantum runs (csrc/fsk_processor_rate_plan.h: processor_ratecvt_start,
    processor_ratecvt_any), and the kernel's walk over its ring from that start, from a stand-alone program under AddressSanitizer
    and UBSan;
  * fskhip_processor_last_tx_kernel is declared, exported and bound, answers "" for a null processor, and the ABI version stays 8;
    FSKHIP_PROC_RATECVT_PAIR has one value in the header, Python and Node;
  * the fused kernel's body and its launcher are each defined once."""
import ctypes as C
import os
import subprocess

from conftest import ROOT


def test_start_arithmetic_under_sanitizers(tmp_path):
    exe = str(tmp_path / "processor_ratecvt_any_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "webaudio_modem_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "processor_ratecvt_any_plan_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_last_tx_kernel_is_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    from webaudio_modem_amd import _lib
    from webaudio_modem_amd.processor import FSKProcessorBatch
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "fskhip_next.h")).read()
    name = "fskhip_processor_last_tx_kernel"
    assert "const char *%s(const fskhip_processor *p);" % name in hdr
    assert hasattr(C.CDLL(_lib.LIB_PATH), name) and name in _lib.SYMBOL_NAMES
    assert L.fskhip_processor_last_tx_kernel(None) == b""
    assert L.fskhip_abi_version() == 8
    assert isinstance(FSKProcessorBatch.last_tx_kernel, property)
    assert "#define FSKHIP_PROC_RATECVT_PAIR 4u" in hdr and _lib.PROC_RATECVT_PAIR == 4
    js = open(os.path.join(ROOT, "napi", "fsk-processor.js")).read()
    dts = open(os.path.join(ROOT, "napi", "fsk-processor.d.ts")).read()
    assert "PROC_RATECVT_PAIR = 4" in js and "get lastTxKernel()" in js
    assert "PROC_RATECVT_PAIR: 4" in dts and "readonly lastTxKernel: string" in dts


def test_the_fused_kernel_and_its_launcher_are_defined_once():
    mod = open(os.path.join(ROOT, "webaudio_modem_amd", "csrc", "fsk_mod.hip")).read()
    launch = open(os.path.join(ROOT, "webaudio_modem_amd", "csrc", "fsk_launch.h")).read()
    assert launch.count("hipError_t launch_processor_io_ratecvt(") == 1 and mod.count("hipError_t launch_processor_io_ratecvt(") == 1
    assert mod.count("void processor_io_ratecvt_kernel(") == 1           # one body for both forms
