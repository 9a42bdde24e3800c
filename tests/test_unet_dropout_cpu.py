"""CPU: tests/unet_dropout_ref.py's restatement of rnr_dropout_draw (Philox4x32-10 known answers, frequency, view-major layout,
the 64-bit counter and key) and the refusals of UNetPlan(dropout=...) that need no device."""
import numpy as np
import pytest

import unet_dropout_ref as ud


def _hex(words):
    return ' '.join('%08x' % int(w) for w in words)


@pytest.mark.parametrize('counter,key,want', [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), 'd16cfe09 94fdcceb 5001e420 24126ea1'),
])
def test_philox_known_answers(counter, key, want):
    assert _hex(ud.philox4x32_10(counter, key)) == want


def test_frequency_of_dropped_elements():
    """2^20 elements at p = 0.1: the number dropped is binomial, mean 104857.6, sigma = sqrt(2^20 0.1 0.9) = 307."""
    m, = ud.draw([(1024, 1024, 0.1)], 1024, 1234, 0)
    dropped = int((m == 0).sum())
    print('dropped %d of 2^20 at p = 0.1' % dropped)
    assert abs(dropped - 104857.6) <= 5 * 307
    assert dropped == 104559                                    # the convention's own figure, recorded with its definition
    kept = np.unique(m[m != 0])
    assert kept.tolist() == [np.float32(1.0) / (np.float32(1.0) - np.float32(0.1))]


def test_multipliers_p0_p1_and_padding():
    a, b, c = ud.draw([(7, 16, 0.0), (5, 16, 1.0), (3, 16, 0.5)], 4, 99, 0)
    assert (a[:, :7] == 1).all() and (a[:, 7:] == 0).all()
    assert (b == 0).all()
    assert set(np.unique(c[:, :3]).tolist()) <= {0.0, 2.0} and (c[:, 3:] == 0).all()


def test_view_major_layout():
    """The tables of the first two views of a 3-view draw are the 2-view draw: a plan sized for more views draws the same masks."""
    layers = [(7, 16, 0.1), (4, 16, 0.5), (130, 144, 0.3)]
    three, two = ud.draw(layers, 3, 42, 1000), ud.draw(layers, 2, 42, 1000)
    for a, b in zip(three, two):
        assert a[:2].tobytes() == b.tobytes()
    assert any((a[2] != a[0]).any() for a in three)


def test_counter_carry_and_high_key_word():
    """Offset 2^32 - 8: block 8 onwards has a non-zero high counter word.  The blocks of a draw that starts at 2^32 equal the
    tail of the one that starts 8 blocks earlier; and the high word of the seed is part of the key."""
    layers = [(64, 64, 0.5)]                                    # 16 blocks per view
    seed = 0x9E3779B97F4A7C15
    early = ud.draw(layers, 2, seed, 2 ** 32 - 8)[0].reshape(-1)
    late = ud.draw(layers, 1, seed, 2 ** 32)[0].reshape(-1)
    assert early[32:96].tobytes() == late.tobytes()
    # without the carry the counter would wrap to (0, 0): another block
    wrapped = ud.draw(layers, 1, seed, 0)[0].reshape(-1)
    assert early[32:96].tobytes() != wrapped.tobytes()
    assert ud.draw(layers, 2, seed & 0xFFFFFFFF, 0)[0].tobytes() != ud.draw(layers, 2, seed, 0)[0].tobytes()
    # int64 bit patterns, as the C ABI takes them, are the same draw
    assert ud.draw(layers, 2, seed - 2 ** 64, 5)[0].tobytes() == ud.draw(layers, 2, seed, 5)[0].tobytes()


def test_step_channels_of_the_network():
    assert ud.unet_step_channels(4, 2) == [4, 4, 8, 8, 8, 8, 8, 4, 4]
    assert len(ud.unet_step_channels(64, 5)) == 21 and max(ud.unet_step_channels(64, 5)) == 512


def test_plan_refuses_dropout_without_training():
    from rnr_amd.unet import UNetPlan
    with pytest.raises(ValueError, match='training=True'):
        UNetPlan({}, 16, 6, 4, 2, (32, 32), 1, 'cuda:0', dropout=[0.1] * 9 + [None])


def test_module_maps_dropout_modules_to_plan_steps():
    """RenderingNet has a Dropout2d behind 21 of its 22 convolutions; eval mode or p = 0 counts as not live."""
    import network
    import torch
    net = network.RenderingNet(nf0=4, in_channels=16, out_channels=6, num_down_unet=5, use_gcn=True).net
    mods = net._step_dropouts()
    assert len(mods) == 22 and mods[-1] is None and all(isinstance(m, torch.nn.Dropout2d) for m in mods[:-1])
    assert len(set(map(id, mods[:-1]))) == 21 and mods[0] is net.in_layer[3]
    net.train()
    assert net._dropout_probs() == (0.1,) * 21 + (0.0,)
    mods[3].eval()
    mods[5].p = 0.0
    assert net._dropout_probs() == tuple(0.0 if i in (3, 5, 21) else 0.1 for i in range(22))
    net.eval()
    assert net._dropout_probs() is None


def test_live_dropout_on_a_cpu_input_is_refused_before_any_device_call():
    """The masks come from the generator of the input's device; with the modules in eval mode the call goes on to the next check."""
    import network
    import torch
    net = network.RenderingNet(nf0=4, in_channels=16, out_channels=6, num_down_unet=2, use_gcn=False).enable_hip_backward()
    net.train()
    with pytest.raises(NotImplementedError, match='generator of a CUDA'):
        net(torch.randn(1, 16, 16, 16, requires_grad=True), None)
