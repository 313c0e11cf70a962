#!/bin/bash
# Debug helper: build devo_amd/lib/libdevo_<tag>.so from the current tree with extra compiler flags on ONE source
# (e.g.  tools/build_variant.sh o2 corr -O2), to A/B kernels inside one GPU run with tools/bench_with_lib.py
# (DEVO_LIB=devo_amd/lib/libdevo_<tag>.so).  The source list, the flags and the compiler are devo_amd.build's.
set -e
tag=$1; src=$2; shift 2
cd "$(dirname "$0")/.."
python -m devo_amd.build > /dev/null
{ read -r HIPCC; read -r -a F; read -r -a SRCS; } < <(python -c 'from devo_amd import build as B; print(B._hipcc()); print(" ".join(B.FLAGS)); print(" ".join(s[:-4] for s in B.SOURCES))')
[[ " ${SRCS[*]} " == *" $src "* ]] || { echo "unknown source '$src' (one of: ${SRCS[*]})" >&2; exit 1; }
"$HIPCC" "${F[@]}" "$@" -c devo_amd/csrc/$src.hip -o devo_amd/lib/${src}_$tag.o
objs=()
for s in "${SRCS[@]}"; do if [ "$s" = "$src" ]; then objs+=("devo_amd/lib/${src}_$tag.o"); else objs+=("devo_amd/lib/$s.o"); fi; done
"$HIPCC" --offload-arch=gfx950 -shared -fPIC -o devo_amd/lib/libdevo_$tag.so "${objs[@]}"
echo devo_amd/lib/libdevo_$tag.so
