# -*- coding: utf-8 -*-
"""python -m yolov4_amd.train / yolov4_amd.val on a COCO tree made of the JPEG fixtures: two epochs of YOLOv4-tiny with
mosaic, the multi-scale schedule (64 and 96 px, a new draw every batch) and the loss statistics in the log; resume,
--evaluate, the validation script, one child process through the module entry; and one model run at 64, 96 and 64 px
again in one process (training step and eval forward), the second visit bit-equal to the first."""
import copy
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import headopt_cases as HO
import recipe
import test_gpu_jpeg as TJ
from yolov4_amd.yolo.data.cocodataset import COCOBatchLoader, COCODataset
from yolov4_amd.yolo.data.multiscale import MultiScale

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
SEED = 5
KEYS = {'epoch', 'ap50', 'ap50_95', 'best_ap50', 'best_ap50_95', 'state_dict', 'optimizer', 'lr_scheduler'}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    import yolov4_amd
    assert yolov4_amd.lib().y4_device_count() >= 1, 'no gfx950 device visible to libyolov4_amd.so'
    return torch.device('cuda:0')


def make_cfg(out_dir, max_epochs=2):
    from yolov4_amd.yolo.model.yolov4_tiny import default_cfg
    return {'DATA': {'MAX_NUM_LABELS': 60, 'BATCH_SIZE': 2, 'WORKERS': 2},
            'AUGMENTATION': dict(TJ.CFG['AUGMENTATION'], IS_MOSAIC=True, RANDOM_RESIZE=True, RANDOM_RESIZE_RANGE=[64, 96],
                                 RANDOM_RESIZE_EVERY=1),
            'MODEL': default_cfg(3),
            'CRITERION': {'TYPE': 'YOLOLoss', 'IGNORE_THRESH': 0.7, 'STATS': True},
            'OPTIMIZER': {'TYPE': 'ADAM', 'LR': 1e-4, 'NO_BIAS': True, 'NO_NORM': True},
            'LR_SCHEDULER': {'TYPE': 'MultiStepLR', 'MILESTONES': [2, 3], 'GAMMA': 0.1, 'IS_WARMUP': True, 'WARMUP_EPOCH': 1,
                             'MULTIPLIER': 1.0},
            'TRAIN': {'IMGSIZE': 64, 'START_EPOCH': 0, 'MAX_EPOCHS': max_epochs, 'ACCUMULATION_STEPS': 1,
                      'OUTPUT_DIR': str(out_dir)},
            'TEST': {'IMGSIZE': 64, 'CONFTHRE': 0.001, 'NMSTHRE': 0.4}}


def write_cfg(path, cfg):
    with open(str(path), 'w') as f:
        json.dump(cfg, f)
    return str(path)


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('coco'))
    TJ.make_tree(root)
    return root


@pytest.fixture(scope='module')
def work(tmp_path_factory):
    return tmp_path_factory.mktemp('work')


@pytest.fixture(scope='module')
def first_run(dev, tree, work):
    """two epochs through main(), in-process: (cfg, cfg path, log lines, what main returned)"""
    from yolov4_amd import train
    cfg = make_cfg(work / 'out')
    path = write_cfg(work / 'cfg.json', cfg)
    lines = []
    ret = train.main([tree, '-c', path, '-p', '1', '-j', '2', '--seed', str(SEED)], log=lines.append)
    return cfg, path, lines, ret


def count_records(labels, model_cfg, layer_no, Fs):
    """positive cells of a layer at iou_thresh 1, the way headopt_cases.assign finds them, with the model's own strides"""
    lab = np.asarray(labels).astype(F32)
    st = model_cfg['STRIDES'][layer_no]
    anc = np.array([(w / st, h / st) for w, h in model_cfg['ANCHORS']], np.float64).astype(F32)
    mask = list(model_cfg['ANCHOR_MASK'][layer_no])
    cells = set()
    for b in range(lab.shape[0]):
        nb = int((lab[b].sum(axis=1, dtype=F32) > 0).sum())
        if not nb:
            continue
        box = lab[b, :nb, :4] / F32(st)
        best = np.argmax(HO.shape_iou32(box[:, 2], box[:, 3], anc), axis=1)
        for t in range(nb):
            i, j = int(box[t, 0].astype(np.int16)), int(box[t, 1].astype(np.int16))
            if 0 <= i < Fs and 0 <= j < Fs and int(best[t]) in mask:
                cells.add((b, mask.index(int(best[t])), j, i))
    return len(cells)


def _train_loader(tree, cfg, multiscale, seed=SEED, img_size=64):
    ds = COCODataset(tree, name='train2017', img_size=img_size, is_train=True, num_classes=3)
    return COCOBatchLoader(ds, 2, cfg, shuffle=True, seed=seed, workers=2, multiscale=multiscale)


# ------------------------------------------------------------------------------------------ the loader
def test_loader_follows_the_schedule_and_none_is_the_fixed_size_loader(dev, tree, work):
    cfg = make_cfg(work / 'unused')
    ms = MultiScale.from_cfg(cfg, seed=SEED)
    assert ms.sizes == (64, 96) and ms.every == 1
    loader = _train_loader(tree, cfg, ms)
    seen = set()
    for epoch in range(3):
        loader.set_epoch(epoch)
        for b, (x, target) in enumerate(loader):
            S = ms.size_at(epoch, b)
            assert tuple(x.shape) == (2, 3, S, S) and loader.last_img_size == S
            seen.add(S)
    assert seen == {64, 96}
    # without a schedule: the dataset's size, per batch, and the batches of a constant schedule of that size bit for bit
    plain, fixed = _train_loader(tree, cfg, None), _train_loader(tree, cfg, MultiScale([64]))
    assert plain.multiscale is None
    a, b = list(plain), list(fixed)
    assert len(a) == len(b) == 2
    for (x1, t1), (x2, t2) in zip(a, b):
        assert tuple(x1.shape) == (2, 3, 64, 64)
        assert torch.equal(x1, x2) and torch.equal(t1['padded_labels'], t2['padded_labels']) and t1['img_info'] == t2['img_info']
    plain.dataset.set_img_size(96)
    assert [tuple(x.shape[2:]) for x, _ in plain] == [(96, 96)] * 2 and plain.last_img_size == 96
    with pytest.raises(ValueError):
        COCOBatchLoader(COCODataset(tree, name='val2017', img_size=64, is_train=False), 2, cfg, multiscale=ms)


# ------------------------------------------------------------------------------------------ main()
LOSS_LINE = re.compile(r'^Epoch: \[(\d+)\]\[(\d+)/(\d+)\].*Loss (\S+) \((\S+)\)\tImgSize: (\d+)x(\d+)$')
STAT_LINE = re.compile(r'^  L(\d): count (\d+)  avg_iou (\S+)  \.5R (\S+)  \.75R (\S+)  obj (\S+)  no_obj (\S+)  cls (\S+)  '
                       r'top1 (\S+)  ign (\d+)$')


def test_main_trains_logs_and_saves(dev, tree, first_run):
    cfg, path, lines, ret = first_run
    out = cfg['TRAIN']['OUTPUT_DIR']
    ckpt = torch.load(os.path.join(out, 'checkpoint.pth.tar'), map_location='cpu', weights_only=True)
    best = torch.load(os.path.join(out, 'model_best.pth.tar'), map_location='cpu', weights_only=True)
    assert set(ckpt) == KEYS and ckpt['epoch'] == 2
    assert set(best) == KEYS and best['epoch'] in (1, 2) and best['ap50'] == ckpt['best_ap50'] == best['best_ap50']
    assert all(bool(torch.isfinite(v).all()) for v in ckpt['state_dict'].values() if v.is_floating_point())
    assert ret == (ckpt['ap50_95'], ckpt['ap50']) and 0.0 <= ret[0] <= 1.0 and 0.0 <= ret[1] <= 1.0
    # the log: per batch one loss line ending in the schedule's size, then one statistics line per layer
    ms = MultiScale.from_cfg(cfg, seed=SEED)
    loader = _train_loader(tree, cfg, ms)
    at = 0
    text = [l for l in lines if LOSS_LINE.match(l) or STAT_LINE.match(l)]
    for epoch in range(2):
        loader.set_epoch(epoch)
        for b, (x, target) in enumerate(loader):
            m = LOSS_LINE.match(text[at])
            assert m, text[at]
            S = ms.size_at(epoch, b)
            assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (epoch + 1, b + 1, 2)
            assert int(m.group(6)) == int(m.group(7)) == S == x.shape[-1]
            assert np.isfinite(float(m.group(4))) and np.isfinite(float(m.group(5)))
            for l, st in enumerate(cfg['MODEL']['STRIDES']):
                s = STAT_LINE.match(text[at + 1 + l])
                assert s and int(s.group(1)) == l, text[at + 1 + l]
                want = count_records(target['padded_labels'].numpy(), cfg['MODEL'], l, S // st)
                assert int(s.group(2)) == want, (epoch, b, l, text[at + 1 + l], want)
            at += 1 + len(cfg['MODEL']['STRIDES'])
    assert at == len(text) == 2 * 2 * 3
    assert sum(int(STAT_LINE.match(l).group(2)) for l in text if STAT_LINE.match(l)) > 0


def test_resume_goes_on_for_exactly_one_more_epoch(dev, tree, work, first_run, monkeypatch):
    from yolov4_amd import train
    from yolov4_amd.yolo.optim.optimizers import build as OB
    cfg, _, _, _ = first_run
    out = cfg['TRAIN']['OUTPUT_DIR']
    before = torch.load(os.path.join(out, 'checkpoint.pth.tar'), map_location='cpu', weights_only=True)
    steps = [int(s['step']) for s in before['optimizer']['state'].values() if 'step' in s]
    assert steps and set(steps) == {4}                         # two epochs of two batches
    cfg3 = make_cfg(work / 'out', max_epochs=3)
    path3 = write_cfg(work / 'cfg3.json', cfg3)
    restored = []
    real = OB.FusedAdam.load_state_dict

    def spy(self, sd):
        real(self, sd)
        restored.append(sorted({int(s['step']) for s in self.state.values() if 'step' in s}))
    monkeypatch.setattr(OB.FusedAdam, 'load_state_dict', spy)
    lines = []
    train.main([tree, '-c', path3, '-p', '1', '-j', '2', '--seed', str(SEED), '--resume', os.path.join(out, 'checkpoint.pth.tar')],
               log=lines.append)
    assert restored == [[4]]                                   # `in`, not hasattr(): the optimizer state came back
    epochs = sorted({int(LOSS_LINE.match(l).group(1)) for l in lines if LOSS_LINE.match(l)})
    assert epochs == [3] and sum(1 for l in lines if LOSS_LINE.match(l)) == 2
    after = torch.load(os.path.join(out, 'checkpoint.pth.tar'), map_location='cpu', weights_only=True)
    assert after['epoch'] == 3 and after['best_ap50'] >= before['best_ap50']
    assert {int(s['step']) for s in after['optimizer']['state'].values() if 'step' in s} == {6}
    assert after['lr_scheduler']['last_epoch'] == before['lr_scheduler']['last_epoch'] + 1
    # the sizes of the third epoch are the schedule's: a resumed run gets what it would have had
    ms = MultiScale.from_cfg(cfg3, seed=SEED)
    assert [int(LOSS_LINE.match(l).group(6)) for l in lines if LOSS_LINE.match(l)] == [ms.size_at(2, 0), ms.size_at(2, 1)]


def test_evaluate_val_and_the_module_entry_agree(dev, tree, work, first_run):
    from yolov4_amd import train, val
    cfg, path, _, _ = first_run
    ckpt = os.path.join(cfg['TRAIN']['OUTPUT_DIR'], 'checkpoint.pth.tar')
    a = train.main([tree, '-c', path, '--resume', ckpt, '--evaluate', '-j', '2'], log=lambda s: None)
    assert len(a) == 2 and all(0.0 <= v <= 1.0 for v in a)
    lines = []
    b = val.main([tree, '-c', path, '-ckpt', ckpt, '-j', '2'], log=lines.append)
    assert tuple(b) == tuple(a)
    assert any('Average Precision' in l for l in lines) or b == (0, 0)
    c = val.main([tree, '-c', path, '-ckpt', ckpt, '-j', '2', '--conf-thre', '-1', '--nms-thre', '-0.5'], log=lambda s: None)
    assert tuple(c) == tuple(a)                                # negative thresholds: the cfg's
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'yolov4_amd.train', tree, '-c', path, '--resume', ckpt, '--evaluate', '-j', '2'],
                       cwd=str(work), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'AP50:95 {:.4f}  AP50 {:.4f}'.format(*a) in r.stdout, r.stdout[-2000:]


def test_ema_run_saves_the_average_and_resumes(dev, tree, work):
    from yolov4_amd import train
    cfg = make_cfg(work / 'ema', max_epochs=1)
    path = write_cfg(work / 'cfg_ema.json', cfg)
    train.main([tree, '-c', path, '-p', '1', '-j', '2', '--ema'], log=lambda s: None)
    file = os.path.join(str(work / 'ema'), 'checkpoint.pth.tar')
    ckpt = torch.load(file, map_location='cpu', weights_only=True)
    assert set(ckpt) == KEYS | {'ema', 'live_state_dict'} and ckpt['ema']['updates'] == 2
    k = next(k for k in ckpt['state_dict'] if k.endswith('conv.weight'))
    assert torch.equal(ckpt['state_dict'][k], ckpt['ema'][k]) and set(ckpt['live_state_dict']) == set(ckpt['state_dict'])
    cfg2 = make_cfg(work / 'ema', max_epochs=2)
    train.main([tree, '-c', write_cfg(work / 'cfg_ema2.json', cfg2), '-p', '1', '-j', '2', '--ema', '--resume', file],
               log=lambda s: None)
    again = torch.load(file, map_location='cpu', weights_only=True)
    assert again['epoch'] == 2 and again['ema']['updates'] == 4


def test_exits_for_more_than_one_process(tree, work, monkeypatch):
    from yolov4_amd import train
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(SystemExit, match='WORLD_SIZE'):
        train.main([tree, '-c', 'does-not-matter.json'])


# ------------------------------------------------------------------------------------------ one model, several sizes
def _model(kind, dev):
    if kind == 'tiny':
        from yolov4_amd.yolo.model.yolov4_tiny import YOLOv4Tiny, default_cfg
        cfg = default_cfg(3)
        model = YOLOv4Tiny(cfg)
    else:
        from yolov4_amd.yolo.model.yolov4 import YOLOv4
        cfg = dict(copy.deepcopy(recipe.MODEL_CFG), N_CLASSES=3)
        model = YOLOv4(cfg, device=dev)
    sd = model.state_dict()
    recipe.fill_state_dict_(sd, 7)
    model.load_state_dict(sd)
    return cfg, model.to(dev)


def _labels(B, S, seed):
    lab = recipe.synth_labels(B, S, seed, counts=[5, 9][:B])
    lab[..., 4] = torch.where(lab[..., 2] > 0, lab[..., 4] % 3, lab[..., 4])
    return lab


@pytest.mark.parametrize('kind', ('tiny', 'full'))
def test_a_size_revisited_gives_the_same_bits(dev, kind):
    """Training forward + loss + backward at 64, at 96, then -- the state put back -- at 64 again: loss, head outputs and
    the first conv's weight gradient of the two visits are torch.equal; likewise an eval forward 64 -> 96 -> 64 (the
    inference filter cache).  No kernel on the path is documented as order-nondeterministic, so nothing here
    is held to a looser bound."""
    from yolov4_amd.yolo.model.yololoss import YOLOLoss
    cfg, model = _model(kind, dev)
    state = {k: v.detach().clone() for k, v in model.state_dict().items()}
    first = next(p for n, p in model.named_parameters() if n.endswith('conv.weight'))
    crit = YOLOLoss(cfg, 0.7, device=dev, mutate_outputs=False, stats=True)

    def step(S):
        model.load_state_dict(state)
        model.train()
        model.zero_grad(set_to_none=True)
        x = recipe.randn((2, 3, S, S), S).to(dev)
        outs = model(x)
        loss = crit(outs, {'padded_labels': _labels(2, S, S)})
        loss.backward()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss))
        return loss.detach().clone(), [o['output'].detach().clone() for o in outs], first.grad.detach().clone()

    a, _, c = step(64), step(96), step(64)
    assert torch.equal(a[0], c[0]) and torch.equal(a[2], c[2])
    assert len(a[1]) == len(c[1]) and all(torch.equal(p, q) for p, q in zip(a[1], c[1]))
    assert a[1][0].shape[2] == 64 // (16 if kind == 'tiny' else 8)

    model.load_state_dict(state)
    recipe.calibrate_bn_(model, recipe.randn((4, 3, 64, 64), 3).to(dev))
    model.eval()

    def infer(S):
        with torch.no_grad():
            out = model(recipe.randn((2, 3, S, S), 100 + S).to(dev)).clone()
        torch.cuda.synchronize()
        return out

    p, q, r = infer(64), infer(96), infer(64)
    assert torch.equal(p, r) and q.shape[1] != p.shape[1]
