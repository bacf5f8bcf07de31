"""CPU tier: the cache policy of the GCN step's HBM streams (fitgnn::NtStream, csrc/common.h) as built into the gfx950 code objects.

tools/nt_probe.py measured every stream with the non-temporal hint and without it (profiles/r05_nt_probe_S-products.log); the
default build carries `nt` on the streams that came out faster and on nothing else:
* the whole-subgraph SpMM's output row stores in the plain launches (layer 1 forward) and the two-hop backward (G) -- not in the
  layer-0 launch over the table, where nt stores were slower;
* the side-table kernel's `prev` loads and ZT stores;
* the segment sum's member row loads (not its stores);
* no window staging load of any launch (all three were 5-7 % slower with nt), no CSR or index load (dword / dwordx2).
"""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "fit-gnn_amd", "lib", "libfitgnn_hip.so")
LLVM = "/opt/rocm/lib/llvm/bin"


@pytest.fixture(scope="module")
def nt_by_kernel(tmp_path_factory):
    """{kernel symbol: [the nt-hinted instructions' mnemonics]} over every gfx950 code object of the library."""
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("ROCm's llvm tools are not installed")
    d = tmp_path_factory.mktemp("co_nt")
    shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, stdout=subprocess.DEVNULL)
    files = sorted(glob.glob(str(d / "lib.so.*gfx950*")))
    assert files, "no gfx950 code object in libfitgnn_hip.so"
    out, symbols = {}, set()
    for f in files:
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", f], check=True, stdout=subprocess.PIPE,
                             text=True).stdout
        name = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
            if m:
                name = m.group(1)
                symbols.add(name)
                continue
            ins = line.split("//")[0].split()
            if name and ins and re.search(r"\bnt\b", " ".join(ins[1:])):
                out.setdefault(name, []).append(ins[0])
    assert any("spmm_block_kernel" in s for s in symbols), "disassembly of the SpMM kernels not found"
    return out


def _one(nt, pattern):
    hits = [k for k in nt if re.search(pattern, k)]
    assert len(hits) <= 1, hits
    return nt[hits[0]] if hits else []


BLOCK = r"spmm_block_kernelIL{}EL{}EL{}EL{}EE"   # <XROW, BWD, NOEPI, TWO>


def test_output_stores_of_the_plain_and_two_hop_launches_are_nt(nt_by_kernel):
    for args in (("b0", "b0", "b1", "b0"), ("b1", "b0", "b1", "b1")):   # layer 1 forward, the two-hop backward
        ins = _one(nt_by_kernel, BLOCK.format(*args))
        assert ins and set(ins) == {"global_store_dwordx4"}, (args, ins)


def test_layer0_table_launch_keeps_the_default_policy(nt_by_kernel):
    assert _one(nt_by_kernel, BLOCK.format("b1", "b0", "b0", "b0")) == []


def test_no_window_staging_or_index_load_is_nt(nt_by_kernel):
    for name, ins in nt_by_kernel.items():
        if "spmm_block_kernel" in name:
            assert not any(i.startswith("global_load") for i in ins), (name, ins)
        assert all(i.endswith("dwordx4") for i in ins), (name, ins)   # 16-byte row accesses only


def test_side_table_kernel_streams_prev_in_and_zt_out(nt_by_kernel):
    ins = _one(nt_by_kernel, r"two_hop_rows_kernel")
    assert "global_load_dwordx4" in ins and "global_store_dwordx4" in ins, ins


def test_segment_sum_loads_members_nt_and_stores_with_the_default(nt_by_kernel):
    ins = _one(nt_by_kernel, r"segment_sum_kernelILi4EE")
    assert ins and set(ins) == {"global_load_dwordx4"}, ins


def test_nt_stays_on_the_probed_kernels(nt_by_kernel):
    allowed = (r"spmm_block_kernel", r"two_hop_rows_kernel", r"segment_sum_kernelILi4EE", r"stream_copy_kernel")
    stray = [k for k in nt_by_kernel if not any(re.search(p, k) for p in allowed)]
    assert not stray, stray
