#!/bin/bash
# Library with cycle stamps: tools/debug/build_trace.sh -DLAFF_GEMM_TRACE [-DLAFF_STRIP_TRACE] [-DLAFF_FCS_TRACE]
#   LAFF_GEMM_TRACE   gemm_nt: per-tile stamps, wait breakdown of the K loop, epilogue stamps
#   LAFF_STRIP_TRACE  sim_strip: per-segment and per-block stamps of wave 0
#   LAFF_FCS_TRACE    fc_strip, fc_strip16: per-segment phase stamps
# Every source is rebuilt with the given macros into scratch/trace/liblaff_hip.so: load it with LAFF_HIP_LIB (the trace_*.py scripts
# hand their stamp buffer over through LAFF_GEMM_TRACE_PTR).  The stamps give correct results, only slower.
set -e
[ $# -gt 0 ] || { echo "usage: $0 -DLAFF_GEMM_TRACE|-DLAFF_STRIP_TRACE|-DLAFF_FCS_TRACE ..." >&2; exit 2; }
cd "$(dirname "$0")/../.."
out=scratch/trace
mkdir -p $out
rm -f $out/*.o
pids=()
for f in $(python3 -c "from laff_amd.build import SOURCES; print(' '.join(s[:-4] for s in SOURCES))"); do
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++20 -fPIC -fno-gpu-rdc "$@" -c laff_amd/csrc/$f.hip -o $out/$f.o &
  pids+=($!)
done
for p in "${pids[@]}"; do wait $p; done
/opt/rocm/bin/hipcc -shared -fPIC --offload-arch=gfx950 -o $out/liblaff_hip.so $out/*.o
echo $out/liblaff_hip.so
