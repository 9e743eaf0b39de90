# Round-3 evidence, one gpurun call:  bash profiles/final_collect.sh   (raw output under gpurun_out/, summaries made afterwards by
# profiles/valu_mix.py + profiles/summarize.py in the build container)
set -e
cd $GRAFT_REPO_ROOT
bash profiles/collect.sh c4
bash profiles/collect_util.sh c4
bash profiles/collect.sh c3 --scene c3 --width 1024 --height 1024 --vthreads 16
bash profiles/collect_util.sh c3 --scene c3 --width 1024 --height 1024 --vthreads 16
O=${PROFILE_OUT:-profile_out}/cfg3; mkdir -p $O
python bench.py --full --scene c2 --width 512 --height 512 --vthreads 4 --steps 1 --warmup 1 > $O/c2.json 2> $O/c2.err
python bench.py --full --scene c3 --width 1024 --height 1024 --vthreads 16 --steps 1 --warmup 1 > $O/c3.json 2> $O/c3.err
python bench.py --full --scene c5 --width 4096 --height 4096 --vthreads 8 --steps 32 --warmup 1 > $O/c5.json 2> $O/c5.err
python bench.py --full > $O/c4.json 2> $O/c4.err
python bench.py --full --host-buffers --no-cpu > $O/c4_host.json 2> $O/c4_host.err
python bench.py --full --no-cpu --opt bvh_builder=0 > $O/c4_hostsah.json 2> $O/c4_hostsah.err
python bench.py --full --no-cpu --opt bvh_builder=1 > $O/c4_lbvh.json 2> $O/c4_lbvh.err
python bench.py --full --no-cpu --simulate-shard 0/8 > $O/c4_shard8.json 2> $O/c4_shard8.err
python bench.py --full --no-cpu --contexts 8 > $O/c4_ctx8.json 2> $O/c4_ctx8.err
python bench.py --full --no-cpu --opt bvh_width=8 > $O/c4_w8.json 2> $O/c4_w8.err
for f in $O/*.json; do python -c "
import json,sys
d=json.load(open('$f')); r=d.get('roofline') or {}; print('$f', d['value'], d['ms_per_step'], r.get('frac'), r.get('trace_Mrays_per_s'), d['config'].get('end_to_end_s'), (d.get('cpu_baseline') or {}).get('value'))"; done
