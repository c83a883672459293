#!/bin/bash
# Registers, scratch and LDS of every kernel of the interpreter's translation units (cross-compiled, no GPU
# needed):
#   tools/kernel_regs.sh [pattern] [extra hipcc flags]
# SPX_TU: the units, default all eleven ("spmv_kernels spmv_xw_kernels spmv_sx_kernels spmv_t_kernels spmv_mv_kernels
# spmv_mv_f32_kernels spmv_mvr_kernels spmv_mvr_f32_kernels spmv_mvsym_kernels scale_kernels sym_scale_kernels"; any other .hip file of
# sparsex_amd/csrc works too).  They compile side by side and leave their assembly in /tmp/spx_asm/<unit>.s
# Names are printed demangled and whole (llvm-cxxfilt of the ROCm tree or c++filt; without either, mangled), less
# the return type, the namespace and the parameter list: csx_spmv_mv_kernel<MvArgs, double, (MvFamily)2, 8, 4> is
# the K = 8, four-wavefront instance of family 2 (MvFamily of spmv_launch.hpp: 0 plain, 1 accum, 2 det).  `pattern`
# is matched against the name as printed.
set -e
cd "$(dirname "$0")/.."
mkdir -p /tmp/spx_asm
units=${SPX_TU:-spmv_kernels spmv_xw_kernels spmv_sx_kernels spmv_t_kernels spmv_mv_kernels spmv_mv_f32_kernels spmv_mvr_kernels spmv_mvr_f32_kernels spmv_mvsym_kernels scale_kernels sym_scale_kernels}
for tu in $units; do
    /opt/rocm/bin/hipcc --offload-arch=gfx950 -std=c++17 -O3 -fPIC -munsafe-fp-atomics -Iinclude -Isparsex_amd/csrc \
        ${2:-} -S --cuda-device-only -o /tmp/spx_asm/$tu.s sparsex_amd/csrc/$tu.hip 2>/dev/null &
done
wait
for tu in $units; do
python3 - "${1:-.}" "$tu" <<'PY'
import re, shutil, subprocess, sys
pat = re.compile(sys.argv[1])
print("# %s" % sys.argv[2])
filt = next((f for f in ("/opt/rocm/llvm/bin/llvm-cxxfilt", shutil.which("llvm-cxxfilt"), shutil.which("c++filt"))
             if f and shutil.which(f)), None)
rows, cur = [], {}
for line in open("/tmp/spx_asm/%s.s" % sys.argv[2]):
    m = re.match(r"\s+\.(name|sgpr_count|vgpr_count|vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|agpr_count):\s+(\S+)", line)
    if not m:
        continue
    k, v = m.groups()
    if k == "name":
        cur = {"name": v}
    cur[k] = v
    if k == "vgpr_spill_count":
        rows.append(cur)
names = [r["name"] for r in rows]
if filt and names:
    names = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
for r, name in zip(rows, names):
    # void spx::kernel<spx::Args, ...>(parameters) -> kernel<Args, ...>
    name = re.sub(r"^void ", "", name).replace("spx::", "").replace("(anonymous namespace)::", "")
    if name.endswith(")"):
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += (name[i] == ")") - (name[i] == "(")
            if depth == 0:
                name = name[:i]
                break
    if pat.search(name):
        print("%-56s vgpr %3s sgpr %3s scratch %4s vspill %3s sspill %3s" % (
            name, r.get("vgpr_count"), r.get("sgpr_count"), r.get("private_segment_fixed_size", "?"),
            r.get("vgpr_spill_count"), r.get("sgpr_spill_count", "?")))
PY
done
