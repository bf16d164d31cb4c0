"""The eligibility predicate of the fused projection-pair BatchNorm node (ops.proj_pair_eligible, Bottleneck.pair_eligible): which
projection bottlenecks run relu(bn3(.) + bn_ds(.)) as ONE node, and which keep the two BatchNorm nodes.  No GPU."""
import pytest

from pylc_amd import ops, runtime
from pylc_amd.nets.encoder_resnet import Bottleneck

OK = dict(fuse=True, training=True, frozen=False, group=None, clamp_eps=False, drop=None, channels=256, fp32_y=True, relu_bits=True,
          needs_grad=True)


def test_eligible_case():
    assert ops.proj_pair_eligible(**OK) is True
    for c in (8, 40, 264, 2048):
        assert ops.proj_pair_eligible(**dict(OK, channels=c))


@pytest.mark.parametrize('change', [dict(fuse=False),                 # PYLC_RUNTIME=fuse_proj_bn=0
                                    dict(training=False),             # eval mode / inference fusion
                                    dict(frozen=True),                # set_bn_frozen(True)
                                    dict(group=object()),             # SyncBN
                                    dict(clamp_eps=True),             # bn_clamp_eps
                                    dict(drop=(0.5, 1)),              # fused dropout
                                    dict(channels=12), dict(channels=4), dict(channels=20),      # C % 8 != 0: no 1-bit mask
                                    dict(fp32_y=False),               # precision mode 3 half activations
                                    dict(relu_bits=False),            # no_relu_bits
                                    dict(needs_grad=False)])          # nothing takes a gradient: no mask is left
def test_every_other_case_takes_the_two_node_path(change):
    assert ops.proj_pair_eligible(**dict(OK, **change)) is False


def test_runtime_knob_defaults_on_and_parses():
    assert runtime.fuse_proj_bn is True
    r = type(runtime)()
    r._apply_overrides('fuse_proj_bn=0')
    assert r.fuse_proj_bn is False
    r._apply_overrides('fuse_proj_bn=1')
    assert r.fuse_proj_bn is True


def test_bottleneck_predicate_follows_module_and_runtime_state():
    blk = Bottleneck(32, 16, 2, 1, True)
    prev = (runtime.fuse_proj_bn, runtime.bn_clamp_eps, runtime.no_relu_bits, runtime.sync_group, runtime.sync_bn)
    try:
        runtime.fuse_proj_bn, runtime.bn_clamp_eps, runtime.no_relu_bits, runtime.sync_group, runtime.sync_bn = True, False, False, None, True
        blk.train()
        assert blk.pair_eligible()
        assert not blk.pair_eligible(needs_grad=False)
        blk.eval()
        assert not blk.pair_eligible()
        blk.train()
        blk.bn3.frozen = True
        assert not blk.pair_eligible()
        blk.bn3.frozen = False
        blk.downsample.child(1).frozen = True
        assert not blk.pair_eligible()
        blk.downsample.child(1).frozen = False
        for name in ('bn_clamp_eps', 'no_relu_bits'):
            setattr(runtime, name, True)
            assert not blk.pair_eligible()
            setattr(runtime, name, False)
        runtime.fuse_proj_bn = False
        assert not blk.pair_eligible()
        runtime.fuse_proj_bn = True
        runtime.sync_group = object()
        assert not blk.pair_eligible()
        runtime.sync_bn = False            # per-GPU statistics: no group reaches the BatchNorms
        assert blk.pair_eligible()
        runtime.sync_group = None
        assert not Bottleneck(32, 3, 1, 1, True).train().pair_eligible()       # C = 12
        assert blk.pair_eligible()
    finally:
        runtime.fuse_proj_bn, runtime.bn_clamp_eps, runtime.no_relu_bits, runtime.sync_group, runtime.sync_bn = prev
