"""Child of tests/test_gpu_tail_exact.py: the library reads NIMG_NO_S2D3_ROWS, NIMG_LATENT_GENERIC, NIMG_LATENT_GENERIC_POW and
NIMG_LATENT_NO_WINDOW once per process, so the forms behind them run here, in a process started with ONE of them set (argv[1] names
it).  Prints the result bytes (hex), one line per tensor; the parent compares them with the float64 reference."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

SWITCHES = ('NIMG_NO_S2D3_ROWS', 'NIMG_LATENT_GENERIC', 'NIMG_LATENT_GENERIC_POW', 'NIMG_LATENT_NO_WINDOW')


def main():
    import numpy as np
    import torch
    switch = sys.argv[1]
    assert switch in SWITCHES and os.environ.get(switch) and not any(os.environ.get(s) for s in SWITCHES if s != switch)
    importlib.import_module('neural-imaging_amd')
    from neural_imaging_amd import _lib, ops
    import tail_cases as C
    _lib.load()
    dev = torch.device('cuda', 0)
    dv = lambda a: torch.from_numpy(np.array(a, dtype=np.float32, order='C')).to(dev).contiguous()
    out = []
    if switch == 'NIMG_NO_S2D3_ROWS':
        for tag, case in (('a', C.S2D3_SWITCH), ('b', C.S2D3_SWITCH2)):
            r = C.s2d3_case(case)
            loss, dz = ops.mse255_sum_s2d3([dv(p) for p in r['parts']], dv(r['a']), dv(r['b']), case['gscale'])
            out += [('loss_' + tag, loss), ('dz_' + tag, dz)]
    else:
        case = C.LATENT_SWITCH
        r = C.latent_case(case)
        ws = ops.LatentWorkspace(case['K'], dev)
        sc = torch.tensor([case['scale']], dtype=torch.float32, device=dev)
        z, cb = dv(r['z']), dv(r['cb'])
        lat, ent = ops.latent_fwd(z, sc, cb, ws, v=case['v'], unit_codebook=case['unit'])
        dscale = torch.zeros(1, device=dev)
        dz = ops.latent_bwd(z, sc, lat, dv(r['dl']), 250.0, cb, ws, dscale=dscale, v=case['v'], unit_codebook=case['unit'])
        out += [('latent', lat), ('entropy', ent), ('dz', dz), ('dscale', dscale)]
    for name, t in out:
        print(name, t.cpu().numpy().tobytes().hex())


if __name__ == '__main__':
    main()
