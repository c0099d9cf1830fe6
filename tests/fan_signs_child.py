"""Child of tests/test_gpu_fan_signs.py: the routes that read a sign plane sit behind switches csrc/ and ops read ONCE per process
(NIMG_TN32_BELOW, NIMG_NO_ACT_SIGN), so they run here, in a process started with exactly the variables the parent names.
argv[1] = 'consumers' | 'fan', argv[2] = the .npz the results go to.  Nothing is compared here; the parent does that."""
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def consumers(ops, dev, results):
    import torch
    import fan_signs_cases as S
    ops.set_compute('bf16')
    for shape in S.CONSUMER_SHAPES:
        for kind in S.OPERAND_KINDS:
            name = S.consumer_name(shape, kind)
            o = S.consumer_operands(shape, kind)
            g = torch.from_numpy(o['gp']).to(dev).to(torch.bfloat16)
            idx, w = torch.from_numpy(o['idx']).to(dev), torch.from_numpy(o['w']).to(dev)
            act = torch.from_numpy(o['act_bits']).to(dev).view(torch.bfloat16)
            plane = torch.from_numpy(S.pack_signs(o['act_bits'])).to(dev)
            results[name + '/mask'] = S.bits(ops.conv2d_dgrad_unpool(g, idx, w, act_mask=act, out_bf16=True))
            results[name + '/sign'] = S.bits(ops.conv2d_dgrad_unpool(g, idx, w, act_mask=act, out_bf16=True, act_sign=plane))
            results[name + '/inverted'] = S.bits(ops.conv2d_dgrad_unpool(g, idx, w, act_mask=act, out_bf16=True, act_sign=~plane))
            print(name, flush=True)


def fan(ops, dev, results):
    import numpy as np
    import torch
    from neural_imaging_amd.models import forensics
    from util import natural_images
    ops.set_compute('bf16')
    x = torch.from_numpy(natural_images(2, 64, 64, seed=5)).to(dev)
    labels = torch.from_numpy(np.array([0, 3], np.int32)).to(dev)
    net = forensics.FAN(n_classes=5, patch_size=64, device=dev)
    probs, ctx = net.forward(x, labels, training=True)
    results['planes'] = np.int64([i for i in range(1, 5) if ctx.get('sign{}'.format(i)) is not None])
    loss, dx = net.backward(ctx, need_input_grad=True)
    torch.cuda.synchronize()
    results['probs'], results['loss'], results['dx'] = probs.cpu().numpy(), loss.cpu().numpy(), dx.cpu().numpy()
    for k, v in net._model.g.items():
        results['grad/' + k] = v.detach().cpu().numpy()


def main():
    import numpy as np
    import torch
    importlib.import_module('neural-imaging_amd')
    from neural_imaging_amd import _lib, ops
    _lib.load()
    results = {}
    {'consumers': consumers, 'fan': fan}[sys.argv[1]](ops, torch.device('cuda', 0), results)
    np.savez_compressed(sys.argv[2], **results)


if __name__ == '__main__':
    main()
