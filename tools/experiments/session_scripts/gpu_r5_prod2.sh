#!/bin/bash
# persistent ring in the planner (PM_C16P default 1): parity tests, per-shape probe and the captured bf16 step against PM_C16P=0 on the same box
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
O=gpurun_out/$1; mkdir -p $O
timeout 900 python -m pytest tests/test_hip_kernels.py -x -q -m gpu -k "conv_bf16 or conv16 or lds_dma" > $O/pytest.log 2>&1; tail -3 $O/pytest.log
echo "== default routing, PM_C16P=0"; PM_C16P=0 PROBE_CONV16=1 timeout 300 python tools/conv16_probe.py 2>&1 | grep -v amdgpu | tee $O/probe_p0.txt
echo "== default routing, persistent ring in the planner"; PROBE_CONV16=1 timeout 300 python tools/conv16_probe.py 2>&1 | grep -v amdgpu | tee $O/probe_p1.txt
for i in 1 2 3; do
  PM_C16P=0 timeout 600 python bench.py --full --no-cpu-baseline --dtype bf16 --no-profile --graph --steps 20 2>/dev/null | tail -1 | python -c "import sys,json; j=json.loads(sys.stdin.read()); print('PM_C16P=0 (graph)', j['ms_per_step'])"
  timeout 600 python bench.py --full --no-cpu-baseline --dtype bf16 --no-profile --graph --steps 20 2>/dev/null | tail -1 | python -c "import sys,json; j=json.loads(sys.stdin.read()); print('default   (graph)', j['ms_per_step'])"
done
