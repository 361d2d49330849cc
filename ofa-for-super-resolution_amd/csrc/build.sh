#!/bin/bash
# Build libofasr_hip.so for gfx950 (MI355X).  hipcc cross-compiles without a GPU.
set -euo pipefail
cd "$(dirname "$0")"
OUT=${1:-libofasr_hip.so}
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -Wall -Wno-unused-function"
objs=()
pids=()
for src in api.hip pixel_shuffle.hip ktransform.hip dwconv.hip pwconv.hip bnact.hip mbconv.hip conv2d.hip conv2d_f32.hip conv_thin.hip mbfused.hip mbfused_f32.hip mbrecal_f32.hip resample.hip tile_io.hip d4.hip add.hip ema.hip quality.hip loss.hip augment.hip degrade.hip yuv.hip reuse.hip route.hip scene.hip resize_scatter.hip mode_io.hip; do
    obj="${src%.hip}.o"
    stale=0                                # no object, or one older than its source or than ANY header of csrc/
    for dep in "$src" *.h ../../include/ofasr.h; do
        if [ ! -f "$obj" ] || [ "$dep" -nt "$obj" ]; then stale=1; fi
    done
    if [ "$stale" = 1 ]; then
        rm -f "$obj"                       # a failed compile must not leave a stale object to link
        hipcc $FLAGS -c "$src" -o "$obj" &
        pids+=($!)
    fi
    objs+=("$obj")
done
for pid in "${pids[@]}"; do wait "$pid"; done   # `wait` without a PID ignores the jobs' exit codes
hipcc --offload-arch=gfx950 -shared -fPIC -o "$OUT" "${objs[@]}"
echo "built $(pwd)/$OUT"
