#!/bin/bash
# Builds libnp2_hip.so (gfx950) in-tree.  hipcc cross-compiles without a GPU.  Translation units are compiled in parallel;
# an object is rebuilt when its source, any header next to it, the C ABI headers or this script changed.
set -e
cd "$(dirname "$0")"
ARCH=${NP2_ARCH:-gfx950}
FLAGS="--offload-arch=$ARCH -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -fno-omit-frame-pointer ${NP2_EXTRA_FLAGS:-}"
SRCS="np2_dense.hip np2_kernels.hip np2_graph.hip np2_passfront.hip np2_cand.hip np2_regions.hip np2_front.hip np2_inflate.hip np2_crc32.hip np2_deflate.hip np2_kcount.hip np2_qv.hip np2_trio.hip np2_bin.hip np2_cmp.hip np2_depth.hip np2_varcall.hip np2_asmcall.hip np2_srqc.hip np2_sradapt.hip np2_rep.hip np2_sam.hip np2_bamin.hip np2_bamout.hip np2_edits.hip np2_map.hip np2_align.hip np2_aligntags.hip np2_alnpack.hip np2_prims.hip np2_ctx.cpp np2_polish.cpp np2_final.cpp np2_vote.cpp np2_shard.cpp np2_io.cpp np2_bamfile.cpp np2_frontend.cpp np2_fetch_gpu.cpp np2_bamread.cpp np2_kcount_host.cpp np2_qv_host.cpp np2_trio_host.cpp np2_bin_host.cpp np2_cmp_host.cpp np2_depth_host.cpp np2_varcall_host.cpp np2_asmcall_host.cpp np2_srqc_host.cpp np2_sradapt_host.cpp np2_rep_host.cpp np2_sam_host.cpp np2_samtail_host.cpp np2_bamin_host.cpp np2_bamout_host.cpp np2_edits_host.cpp np2_map_host.cpp np2_alnpack_host.cpp np2_deflate_host.cpp np2_batch.cpp"
mkdir -p obj
pids=()
objs=()
for f in $SRCS; do
  [ -f "$f" ] || continue
  o=obj/${f%.*}.o
  objs+=("$o")
  stale=0
  [ -f "$o" ] || stale=1
  for d in "$f" *.hpp ../../include/*.h build.sh; do [ "$d" -nt "$o" ] && stale=1; done
  if [ $stale = 1 ]; then
    echo "hipcc $f"
    hipcc $FLAGS -x hip -c "$f" -o "$o" &
    pids+=($!)
  fi
done
rc=0
for p in "${pids[@]}"; do wait "$p" || rc=1; done
[ $rc = 0 ] || { echo "build failed"; exit 1; }
hipcc --offload-arch=$ARCH -shared -fPIC -o ../libnp2_hip.so "${objs[@]}" -lz -lpthread -rdynamic
echo "built nextpolish2_amd/libnp2_hip.so"
