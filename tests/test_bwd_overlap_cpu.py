"""The arithmetic behind the co-run launch of the backward's transposed aggregation (host.h: kAggCorunLds, kAggCorunVgprs), held
against the compiler's own metadata of the two kernels that share a CU: nothing here needs a GPU."""
import importlib.util
import os
import re
import shutil

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_PER_CU = 160 * 1024        # MI355X
VGPRS_PER_SIMD = 512
DW = "kan_split_dw_kernel<3,false,1,4,false,false>"          # the headline layer's weight gradient
CORUN = "agg_rows_v4_corun_kernel<16>"


def _constant(name):
    text = open(os.path.join(ROOT, "kagnn_amd", "csrc", "host.h")).read()
    m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", text)
    assert m, name
    return int(eval(m.group(1), {"__builtins__": {}}))


def _alloc(vgprs):
    return -(-vgprs // 8) * 8          # the hardware's allocation granule


def test_four_corun_workgroups_and_one_weight_gradient_wave_fit_whatever_starts_first():
    objdir = os.path.join(ROOT, "kagnn_amd", "lib", "obj")
    if not os.path.isdir(objdir) or not shutil.which("c++filt") or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no build objects / LLVM tools on this machine (the library was shipped prebuilt)")
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    rows = {k["demangled"]: k for k in kr.collect(objdir)}
    assert DW in rows and CORUN in rows, sorted(rows)[:5]
    lds, cap = _constant("kAggCorunLds"), _constant("kAggCorunVgprs")
    dw, agg = rows[DW], rows[CORUN]
    # the row kernel stays inside the register budget the launch was sized for, without spilling and without LDS of its own
    assert _alloc(agg["vgpr_count"]) <= cap, agg
    assert agg.get("vgpr_spill_count", 0) == 0 and agg.get("private_segment_fixed_size", 0) == 0
    assert agg.get("group_segment_fixed_size", 0) == 0
    # LDS: four requests fit a CU beside a weight-gradient workgroup, five do not even alone
    assert 4 * lds + dw.get("group_segment_fixed_size", 0) <= LDS_PER_CU < 5 * lds
    # registers: a 256-thread workgroup is one wave per SIMD, so four workgroups are four waves beside the weight gradient's one
    assert 4 * cap + _alloc(dw["vgpr_count"]) <= VGPRS_PER_SIMD
    assert _alloc(dw["vgpr_count"]) > VGPRS_PER_SIMD // 2          # one weight-gradient wave per SIMD: what the launch assumes
