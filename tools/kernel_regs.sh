#!/bin/bash
# Registers, scratch and LDS of every kernel of the interpreter's translation units (cross-compiled, no GPU
# needed):
#   tools/kernel_regs.sh [pattern] [extra hipcc flags]
# SPX_TU: the units, default all five ("spmv_kernels spmv_xw_kernels spmv_sx_kernels spmv_mv_kernels
# spmv_mvsym_kernels"; any other .hip file of sparsex_amd/csrc works too).  They compile side by side and leave their assembly in
# /tmp/spx_asm/<unit>.s
set -e
cd "$(dirname "$0")/.."
mkdir -p /tmp/spx_asm
units=${SPX_TU:-spmv_kernels spmv_xw_kernels spmv_sx_kernels spmv_mv_kernels spmv_mvsym_kernels}
for tu in $units; do
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -std=c++17 -O3 -fPIC -munsafe-fp-atomics -Iinclude -Isparsex_amd/csrc \
        ${2:-} -S --cuda-device-only -o /tmp/spx_asm/$tu.s sparsex_amd/csrc/$tu.hip 2>/dev/null &
done
wait
for tu in $units; do
python3 - "${1:-.}" "$tu" <<'PY'
import re, sys
pat = re.compile(sys.argv[1])
print("# %s" % sys.argv[2])
cur = {}
for line in open("/tmp/spx_asm/%s.s" % sys.argv[2]):
    m = re.match(r"\s+\.(name|sgpr_count|vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|agpr_count):\s+(\S+)", line)
    if not m:
        continue
    k, v = m.groups()
    if k == "name":
        cur = {"name": v}
    cur[k] = v
    if k == "vgpr_spill_count" and pat.search(cur["name"]):
        name = re.sub(r"^_ZN3spx\d+", "", cur["name"])[:48]
        print("%-48s vgpr %3s sgpr %3s scratch %4s vspill %3s sspill %3s" % (
            name, cur.get("vgpr_count"), cur.get("sgpr_count"), cur.get("private_segment_fixed_size", "?"),
            cur.get("vgpr_spill_count"), cur.get("sgpr_spill_count", "?")))
PY
done
