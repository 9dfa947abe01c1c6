#!/bin/bash
# tools/build_variant.sh <name> <-D flags...>: the engine built with other compile-time constants into fastsk_amd/lib/lib<name>.so
set -e
NAME=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
O=$R/fastsk_amd/lib/obj_$NAME; mkdir -p $O
for u in $R/fastsk_amd/csrc/*.hip; do  # (every unit of the engine: a list here went stale)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -pthread "$@" -c $u -o $O/$(basename $u .hip).o &
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -c $R/fastsk_amd/csrc/fsk_fasta.cpp -o $O/fsk_fasta.o &
wait
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -pthread $O/*.o -ldl -o $R/fastsk_amd/lib/lib$NAME.so
rm -rf $O
echo built $R/fastsk_amd/lib/lib$NAME.so
