#!/bin/bash
# Builds A/B variants of the library (compile-time knobs) into abv/
# for tools/gpu_variants.sh; the product library is built by __graft_entry__.build().
# The bounding sources (pdp_bound*.hip) are recompiled per variant, with the
# variant's flags; the other sources are compiled once (build/abv_common/) and
# linked into every variant.
set -e
cd "$(dirname "$0")/.."
mkdir -p abv build/abv_common
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -munsafe-fp-atomics -I include"
CSRC=pipelinedp_amd/csrc
common=()
for src in $CSRC/*.hip; do
  case $(basename $src) in pdp_bound*.hip) continue ;; esac
  obj=build/abv_common/$(basename $src .hip).o
  if [ ! -f $obj ] || [ $src -nt $obj ] || [ -n "$(find $CSRC include -name '*.h' -newer $obj)" ]; then
    /opt/rocm/bin/hipcc $FLAGS -c $src -o $obj &
  fi
  common+=($obj)
done
wait
# a variant named NAME builds abv_src/NAME/<file> instead of a bounding source
# when that file exists (e.g. an older revision: git show REV:pipelinedp_amd/csrc/<file>);
# the headers beside it are the current ones unless abv_src/NAME/ has its own
build() {
  local objs=() src obj h
  for src in $CSRC/pdp_bound*.hip; do
    if [ -f abv_src/$1/$(basename $src) ]; then
      for h in $CSRC/*.h; do [ -f abv_src/$1/$(basename $h) ] || cp $h abv_src/$1/; done
      src=abv_src/$1/$(basename $src)
    fi
    obj=build/abv_common/$(basename $src .hip)_$1.o
    /opt/rocm/bin/hipcc $FLAGS "${@:2}" -c $src -o $obj &
    objs+=($obj)
  done
  wait
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o abv/$1.so "${objs[@]}" "${common[@]}"
}
for spec in "$@"; do
  name=${spec%%:*}; flags=${spec#*:}
  [ "$name" = "$spec" ] && flags=""
  build $name $flags &
done
wait
ls -la abv
