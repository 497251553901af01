"""Records tests/golden/step_launches.json, the goldens of tests/test_gpu_step_launches.py, from the library the package loads (G4R_LIB
selects another): run it at the commit whose behaviour is to be kept.  Every case is recorded twice; a case whose two unprofiled runs
give different bits gets a null digest (and is named on stdout), one whose kernel choice or launch counts differ stops the recorder.

    python tools/record_step_launches.py [--out FILE] [case ...]
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import step_launch_cases as slc      # noqa: E402


def main(argv):
    out = slc.GOLDEN
    if '--out' in argv:
        k = argv.index('--out')
        out = argv[k + 1]
        argv = argv[:k] + argv[k + 2:]
    names = argv or list(slc.CASES)
    golden = {}
    if argv and os.path.exists(out):
        golden = json.load(open(out))
    unstable = []
    for name in names:
        a, b = slc.record(name), slc.record(name)
        if {k: v for k, v in a.items() if k != 'digest'} != {k: v for k, v in b.items() if k != 'digest'}:
            raise SystemExit('%s: kernel choice / launch counts differ between two runs: %r | %r' % (name, a, b))
        if a['digest'] != b['digest']:
            unstable.append(name)
            a['digest'] = None
        golden[name] = a
        print('%-45s n_cu %d digest %s launches %s' % (name, a['n_cu'], (a['digest'] or 'NOT REPRODUCIBLE')[:16], a.get('launches')), flush=True)
        with open(out, 'w') as f:
            json.dump(golden, f, indent=1, sort_keys=True)
            f.write('\n')
    print('cases without a digest: %s' % (unstable or 'none'))
    bad = [n for n in unstable if n in slc.MANDATORY]
    if bad:
        print('MANDATORY cases that do not repeat their bits: %s' % bad)
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
