"""CPU suite: the host side of frozen BatchNorm (DeepLab(freeze_bn=True)) -- the Meta field and its way through
checkpoints, the module flags and their train() / eval() round trips, unchanged state-dict keys, the refusals, the C ABI's argument
checks (made on the host before any launch)."""
import json
import os

import pytest
import torch

HERE = os.path.join(os.path.dirname(__file__), 'golden')


def _flags(net):
    from pylc_amd.layers import BatchNorm2d, Conv2d, DepthwiseConv3x3
    bns = [m.frozen for m in net.modules() if isinstance(m, BatchNorm2d)]
    convs = [m.bn_frozen for m in net.modules() if isinstance(m, (Conv2d, DepthwiseConv3x3))]
    return bns, convs


def test_meta_field_and_unknown_fields():
    from pylc_amd.model import Meta
    assert Meta().freeze_bn is False
    assert Meta(freeze_bn=True).freeze_bn is True
    m = Meta()
    m.update({'freeze_bn': True, 'not_a_field': 1})
    assert m.freeze_bn is True and not hasattr(m, 'not_a_field')


def test_checkpoint_carries_the_flag_and_old_files_load_with_false(tmp_path):
    from pylc_amd.model import Model, Meta
    from pylc_amd import checkpoint as ck
    m = Model(Meta(arch='deeplab', backbone='xception', n_classes=4, ch=1, freeze_bn=True), 'cpu').build()
    assert m.net.freeze_bn is True
    path = str(tmp_path / 'checkpoint.pth')
    ck.save(m, path)
    raw = ck.load_reference_file(path)
    assert raw['meta'].freeze_bn is True
    assert ck.meta_from_reference(raw['meta']).freeze_bn is True
    assert list(raw['model']) == list(m.net.state_dict())
    # a file written before the field existed: its meta has no such attribute
    del raw['meta'].__dict__['freeze_bn']
    old = ck.meta_from_reference(raw['meta'])
    assert old.freeze_bn is False and old.backbone == 'xception' and old.n_classes == 4
    # ... and the committed reference-written checkpoint (no such field either)
    ref = ck.load_reference_file(os.path.join(HERE, 'ref_checkpoint_tiny.pth'))
    assert not hasattr(ref['meta'], 'freeze_bn') and ck.meta_from_reference(ref['meta']).freeze_bn is False
    m2 = Model(ck.meta_from_reference(ck.load_reference_file(path)['meta']), 'cpu').build()
    assert m2.net.freeze_bn is True and all(_flags(m2.net)[0])
    ck.load_into(m2, path, resume=True)
    assert m2.net.freeze_bn is True and all(_flags(m2.net)[0])


@pytest.mark.parametrize('backbone', ['resnet', 'xception'])
def test_set_bn_frozen_and_mode_round_trips(backbone):
    import pylc_amd
    from pylc_amd.layers import BatchNorm2d
    net = pylc_amd.DeepLab(backbone=backbone, n_classes=5)
    bns, convs = _flags(net)
    assert net.freeze_bn is False and len(bns) > 50 and not any(bns) and not any(convs)
    assert BatchNorm2d(8).frozen is False
    assert net.set_bn_frozen(True) is net
    bns, convs = _flags(net)
    assert net.freeze_bn is True and all(bns) and all(convs)
    for mode in (net.eval, net.train, net.eval, net.train):
        mode()
        bns, convs = _flags(net)
        assert net.freeze_bn is True and all(bns) and all(convs)
    assert net.training and all(m.training for m in net.modules())        # still train() mode: dropout, gradients
    net.set_bn_frozen(False)
    bns, convs = _flags(net)
    assert net.freeze_bn is False and not any(bns) and not any(convs)
    net2 = pylc_amd.DeepLab(backbone=backbone, n_classes=5, freeze_bn=True)
    assert net2.freeze_bn is True and all(_flags(net2)[0]) and all(_flags(net2)[1])


@pytest.mark.parametrize('tag,kw', [('deeplab_resnet', dict(backbone='resnet', n_classes=9)),
                                    ('deeplab_xception', dict(backbone='xception', n_classes=11))])
def test_state_dict_keys_unchanged(tag, kw):
    import pylc_amd
    keys = json.load(open(os.path.join(HERE, tag + '.json')))['keys']
    net = pylc_amd.DeepLab(freeze_bn=True, **kw)
    assert [(k, list(v.shape)) for k, v in net.state_dict().items()] == [(k, list(s)) for k, s in keys]
    plain = pylc_amd.DeepLab(**kw)
    plain.load_state_dict(net.state_dict())                       # strict: nothing extra, nothing missing
    assert 'frozen' not in ' '.join(net.state_dict())
    assert all(int(v) == 0 for k, v in net.state_dict().items() if k.endswith('num_batches_tracked'))


def test_unet_refuses_freeze_bn():
    from pylc_amd.model import Model, Meta
    with pytest.raises(ValueError, match='freeze_bn.*unet'):
        Model(Meta(arch='unet', freeze_bn=True), 'cpu').build()
    Model(Meta(arch='unet', freeze_bn=False, n_classes=4), 'cpu').build()


def test_frozen_bwd_argument_checks_need_no_gpu():
    """pylc_bn_frozen_bwd validates on the host before any launch, like its siblings."""
    import ctypes as C
    from pylc_amd.lib import lib, BnExtra
    p = C.c_void_p(64)                                              # never dereferenced: every call below is refused

    def call(m=8, c=8, relu=0, out=None, scale=None, shift=None, sums=None, ws=None, ex=None, dy_pitch=None, y=p):
        return lib.pylc_bn_frozen_bwd(p, c, out, c if out else 0, y, c, p, p, p, m, c, relu, p, c if dy_pitch is None else dy_pitch,
                                      None, 0, None, scale, shift, sums, ws, ex, None)
    assert call(c=6) != 0 and b'C % 4' in lib.pylc_last_error()
    assert call(m=0) != 0 and b'M > 0' in lib.pylc_last_error()
    assert call(dy_pitch=4) != 0 and b'pitch' in lib.pylc_last_error()
    assert call(relu=1) != 0 and b'relu needs' in lib.pylc_last_error()
    assert call(sums=p) != 0 and b'together' in lib.pylc_last_error()
    assert call(sums=p, ws=p, y=None) != 0 and b'y (pitch' in lib.pylc_last_error()
    ex = BnExtra()
    ex.nplanes, ex.dy_planes, ex.dy_bound = 2, 64, 64
    assert call(ex=C.byref(ex)) != 0 and b'fp32 operands only' in lib.pylc_last_error()
    ex = BnExtra()
    ex.nplanes, ex.relu_mask = 2, 64
    assert call(c=12, relu=1, ex=C.byref(ex)) != 0 and b'C % 8' in lib.pylc_last_error()
