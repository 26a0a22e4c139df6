#!/bin/bash
# GPU box: the C++ host loop on the three reference workloads, four frames in flight and one (us per frame).
# usage: tools/quick.sh [tag]
EXE=pixel-art-raytracer_amd/lib/par_pipeline
tag=${1:-quick}
for k in 4 1; do
  f=$($EXE --scene floor --size 4096 --frames 300 --inflight $k --threads $k | head -1)
  s=$($EXE --size 4096 --prims 1024 --frames 4000 --inflight $k --threads $k | head -1)
  g=$($EXE --scene graybox --frames 6000 --inflight $k --threads $k | head -1)
  python3 - "$tag" "$k" "$f" "$s" "$g" <<'PY'
import json, sys
tag, k = sys.argv[1], sys.argv[2]
v = [json.loads(x)["us_per_frame"] for x in sys.argv[3:6]]
print(f"{tag} inflight {k}: floor {v[0]:.1f} us  headline {v[1]:.2f} us  graybox {v[2]:.2f} us")
PY
done
