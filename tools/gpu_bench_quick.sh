set -o pipefail
timeout -k 10 300 python bench.py --full --no-cpu-baseline --chain-captures 0 | tail -1 | python3 -c "
import json, sys
d=json.loads(sys.stdin.read())
print(d['value'], d['roofline']['frac']); print(d.get('bit_exact_engine')); print(d.get('vector_engine',{}).get('Msamples_per_s_per_gpu'))
"
