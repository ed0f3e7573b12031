#!/bin/bash
# one GPU-box visit: GPU test-suite + the three bench workloads (--full lines); stops at the first step that fails
# usage: [OUT=DIR] bash tools/gpu_round.sh [more bench.py options]   (outputs under DIR, default a fresh temporary directory)
O=${OUT:-$(mktemp -d /tmp/orbx_round.XXXXXX)}
mkdir -p $O; echo "outputs under $O"
timeout -k 10 1200 python3 -m pytest tests -m gpu -x -q > $O/pytest.log 2>&1; rc=$?; echo "pytest rc=$rc"; tail -15 $O/pytest.log
[ $rc = 0 ] || exit $rc
for wl in euroc kitti tumvi; do
  timeout -k 10 600 python3 bench.py --full --workload $wl "$@" > $O/bench_$wl.json 2> $O/bench_$wl.err; rc=$?; echo "bench $wl rc=$rc"
  tail -c 1500 $O/bench_$wl.err; cut -c1-900 $O/bench_$wl.json
  [ $rc = 0 ] || exit $rc
done
# the OpenCV pin: the first box that has cv2 generates the goldens tests/test_oracle_vs_opencv.py waits for
python3 -c "import cv2; print('cv2', cv2.__version__)" 2>/dev/null && python3 tools/gen_ocv_golden.py && echo "OpenCV goldens written: commit tests/golden/ocv_*.npz" || echo "cv2: not importable on this box"
