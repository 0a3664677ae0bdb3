#!/bin/bash
# Build a variant libmisort with build-time switches for A/B probes:
#   tools/build_variant.sh NAME "-DMISORT_MK_NT=256"
# -> parallel-computing-mpi_amd/lib/variants/libmisort_NAME.so (bench: MISORT_LIBRARY=...)
set -e
HERE="$(cd "$(dirname "$0")/.." && pwd)"
C="$HERE/parallel-computing-mpi_amd/csrc"; L="$HERE/parallel-computing-mpi_amd/lib"; O="$L/variants/$1"
mkdir -p "$O"
F="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -I$HERE/include -I$C $2"
# every kernel source of libmisort.so (csrc/Makefile); runtime.o is the default build's
SRCS="kernels sort_u32 sort_u64 codec pairs rows rows_u32 rows_u64 rows_pairs segs segs_u32 segs_u64 runs runsk runsk_fg6"
pids=""
for src in $SRCS; do
  /opt/rocm/bin/hipcc $F -c "$C/$src.hip" -o "$O/$src.o" &
  pids="$pids $!"
done
for p in $pids; do wait "$p"; done
OBJS=""
for src in $SRCS; do OBJS="$OBJS $O/$src.o"; done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o "$L/variants/libmisort_$1.so" $OBJS "$L/runtime.o" \
  -L/opt/rocm/lib -lrccl -Wl,-rpath,/opt/rocm/lib
rm -rf "$O"
