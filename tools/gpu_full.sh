#!/bin/bash
# Round-end check on one box: the whole -m gpu suite, smoke(), the driver's bench command (timed), kernel stats of the same build.
TAG=${1:-r06_j}
export PYTHONUNBUFFERED=1
R=$PWD; O=$R/gpurun_out/$TAG; mkdir -p $O
timeout 1500 python -m pytest tests -m gpu -q -x > $O/pytest.log 2>&1; echo "pytest rc=$?"; tail -4 $O/pytest.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1; echo "smoke rc=$?"; tail -2 $O/smoke.log
S=$(date +%s)
timeout 900 python bench.py --full --gpus 1 --steps 20 --warmup 5 > $O/bench.json 2> $O/bench.err; echo "bench rc=$? in $(( $(date +%s) - S )) s"
cut -c1-300 $O/bench.json
