"""Child of tests/test_gpu_conv_switches.py: csrc/ reads most NIMG_* switches of the convolution files ONCE per process, and a stream
that nimg_bind_tickets has bound keeps the ticket finish for the rest of its process, so the forms behind them run here, in a
process started with exactly one group's variables set.  argv[1] names the group (conv_cases.GROUPS), argv[2] the directory the
results go to: every result tensor of every case in <dir>/<group>.npz under '<case>/<key>' - in the ticket groups also the whole
counter buffer of every bound stream after each case ('<case>/tickets') and how many streams are bound ('<case>/bound_streams').  One line per case says which ops call was made.  Nothing
is compared here; the parent does that against the float64 reference."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import numpy as np
    import torch
    import conv_cases as C
    group, out_dir = sys.argv[1], sys.argv[2]
    want = C.GROUPS[group]['env']
    have = {k: v for k, v in os.environ.items() if k.startswith('NIMG_')}
    assert have == want, 'group {}: NIMG_* variables {} set, {} wanted'.format(group, have, want)
    importlib.import_module('neural-imaging_amd')
    from neural_imaging_amd import _lib, ops
    _lib.load()
    dev = torch.device('cuda', 0)
    tickets = group in C.TICKET_GROUPS
    assert ops.TICKETS == tickets
    results = {}
    for case in C.GROUPS[group]['cases']:
        tensors, what = C.run(case, ops, dev)
        for key, t in tensors:
            results[case['name'] + '/' + key] = C.host(t)
        if tickets:
            torch.cuda.synchronize()
            assert len(ops._TICKETS) > 0, 'no stream was bound'
            results[case['name'] + '/tickets'] = torch.cat([b.reshape(-1) for b in ops._TICKETS.values()]).cpu().numpy()
            results[case['name'] + '/bound_streams'] = np.int64([len(ops._TICKETS)])
        print('{}: {}'.format(case['name'], what), flush=True)
    np.savez_compressed(os.path.join(out_dir, group + '.npz'), **results)


if __name__ == '__main__':
    main()
