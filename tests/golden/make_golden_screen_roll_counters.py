"""Regenerates tests/golden/screen_roll_counters.json: the `stats` counters of cg_pointmlp_max_screened on the cases of
tests/test_pointmlp_screen_roll_gpu.py, as the loaded library gives them.  Run from the repository root on an MI355X, with the
library of the commit whose screen is the yardstick (CATGRASP_AMD_LIB selects a build):

    python tests/golden/make_golden_screen_roll_counters.py

The file holds settings and recorded numbers only.  The committed one was recorded with the library of the commit before the
screen became a rolling pipeline over the channel blocks; each case's output bits are compared with the exact entry's on the way."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
sys.path.insert(0, os.path.join(HERE, '..', '..'))
import test_pointmlp_screen_roll_gpu as R  # noqa: E402


def main():
    cases = {key: R.measure_counters(key) for key in sorted(R.counter_cases())}
    for key, c in cases.items():
        print(key, c, flush=True)
    doc = {'settings': {'B': R.T.B_BIG, 'gains': list(R.T.GAINS), 'counters': list(R.T.COUNTERS), 'forces': [0, 2],
                        'block_scales': R.BLOCK_SCALES},
           'cases': cases}
    out = sys.argv[1] if len(sys.argv) > 1 else R.GOLDEN
    with open(out, 'w') as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write('\n')
    print(out, os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
