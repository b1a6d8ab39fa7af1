"""go_slam_amd/weight_packs.py (one key over live tensors, one cache class) and its wiring into the tracker's modules, on CPU
tensors: every test fails on a cache that serves a value derived from weights that are no longer the module's."""
import copy
import gc
import pickle
import weakref

import pytest
import torch
import torch.nn as nn

from go_slam_amd.weight_packs import WeightPacks, tensors_key


def _counting(conv, calls):
    def build():
        calls.append(1)
        return conv.weight.detach().clone(), conv.bias.detach().clone()
    return build


def _get(cache, conv, calls, kind="nhwc"):
    return cache.get((weakref.ref(conv), kind), (conv.weight, conv.bias), _counting(conv, calls))


def test_unchanged_conv_builds_once():
    cache, conv, calls = WeightPacks(), nn.Conv2d(4, 8, 3), []
    a = _get(cache, conv, calls)
    b = _get(cache, conv, calls)
    assert len(calls) == 1 and a is b


def _write_weight(conv):
    with torch.no_grad():
        conv.weight.mul_(2.0)


def _write_bias(conv):
    with torch.no_grad():
        conv.bias.add_(1.0)


def _rebind_data(conv):
    conv.weight.data = torch.randn_like(conv.weight)


def _replace_parameter(conv):
    conv.weight = nn.Parameter(torch.randn_like(conv.weight))


def _load_assign(conv):
    conv.load_state_dict({k: torch.randn_like(v) for k, v in conv.state_dict().items()}, assign=True)


@pytest.mark.parametrize("change", [_write_weight, _write_bias, _rebind_data, _replace_parameter, _load_assign])
def test_every_kind_of_weight_change_rebuilds(change):
    cache, conv, calls = WeightPacks(), nn.Conv2d(4, 8, 3), []
    _get(cache, conv, calls)
    change(conv)
    w, b = _get(cache, conv, calls)
    assert len(calls) == 2 and torch.equal(w, conv.weight) and torch.equal(b, conv.bias)
    _get(cache, conv, calls)
    assert len(calls) == 2


def test_pack_kinds_of_one_conv_do_not_alias():
    cache, conv = WeightPacks(), nn.Conv2d(4, 8, 1)
    a = cache.get((weakref.ref(conv), "1x1"), (conv.weight, conv.bias), lambda: "fragments")
    b = cache.get((weakref.ref(conv), "nhwc"), (conv.weight, conv.bias), lambda: "copy")
    assert (a, b) == ("fragments", "copy")
    assert cache.get((weakref.ref(conv), "1x1"), (conv.weight, conv.bias), lambda: "again") == "fragments"


def test_multi_tensor_pack_rebuilds_when_any_member_changes():
    cache, calls = WeightPacks(), []
    ts = [torch.randn(6) for _ in range(4)]

    def get():
        return cache.get("merged", ts, lambda: calls.append(1) or torch.cat(ts))
    get()
    for i in range(len(ts)):                                # the last member included
        ts[i].add_(1.0)
        assert torch.equal(get(), torch.cat(ts)) and len(calls) == 2 + 2 * i
        ts[i].data = torch.randn(6)                         # .data rebound: same object, same version, other memory
        assert torch.equal(get(), torch.cat(ts)) and len(calls) == 3 + 2 * i
    get()
    assert len(calls) == 1 + 2 * len(ts)


def test_changes_that_cancel_in_a_sum_still_change_the_key():
    """version +1 on one tensor, and a second tensor rebound to memory whose address differs by -1: the sums of versions
    + addresses agree before and after, the key does not (uint8 views of one buffer give addresses one byte apart)"""
    buf = torch.zeros(64, dtype=torch.uint8)
    a, b = torch.zeros(3), buf[9:17]
    before = tensors_key((a, b))
    a.add_(1.0)
    b.data = buf[8:16]
    after = tensors_key((a, b))
    assert isinstance(after, tuple) and after != before
    assert after[0] != before[0] and after[1] != before[1]  # each tensor's own part moved
    total = lambda key: sum(part[0] + part[1] for part in key)
    assert total(after) == total(before)                    # ... although a sum would not have seen it


def test_entries_do_not_keep_replaced_modules_or_parameters_alive():
    cache, calls = WeightPacks(), []
    seq = nn.Sequential(nn.Conv2d(4, 8, 3))
    _get(cache, seq[0], calls)
    old_module, old_weight = weakref.ref(seq[0]), weakref.ref(seq[0].weight)
    seq[0] = nn.Conv2d(4, 8, 3)
    gc.collect()
    assert old_module() is None and old_weight() is None
    _get(cache, seq[0], calls)                              # the dead module's entry leaves at the next rebuild
    assert len(calls) == 2 and len(cache._entries) == 1
    old_weight = weakref.ref(seq[0].weight)
    seq[0].weight = nn.Parameter(torch.randn(8, 4, 3, 3))
    _get(cache, seq[0], calls)
    gc.collect()
    assert old_weight() is None and len(calls) == 3


def _fresh_state(module):
    return {k: torch.randn_like(v) for k, v in module.state_dict().items()}


def test_conv_gru_packs_follow_its_weights():
    """_half_weights(), _hw_hoist, _ww_pack and _weights_key() after load_state_dict and after replacing the parameter of
    a member that is not the first one (the z|r weight is cat(convz, convr): rows 128: are convr's)"""
    from go_slam_amd.droid_net import ConvGRU
    gru = ConvGRU(128, 320)
    hw, key = gru._half_weights(), gru._weights_key()
    assert gru._half_weights() is hw and gru._weights_key() == key
    gru.load_state_dict(_fresh_state(gru))
    hw2, key2 = gru._half_weights(), gru._weights_key()
    assert key2 != key and torch.equal(hw2[0][128:], gru.convr.weight.half())
    assert torch.equal(hw2[6][5], gru.convq_glo.bias)       # the last member of the pack
    assert torch.equal(gru._hw_hoist[0][128:256], gru.convr.weight[:, 128:256].half())
    gru.convr.weight = nn.Parameter(torch.randn_like(gru.convr.weight))
    assert gru._weights_key() != key2 and torch.equal(gru._half_weights()[0][128:], gru.convr.weight.half())
    key3 = gru._weights_key()
    gru.convq_glo.bias.data = torch.randn(128)              # .data of the last member: no version moves
    assert gru._weights_key() != key3 and torch.equal(gru._half_weights()[6][5], gru.convq_glo.bias)
    gru.w.weight.data = torch.randn_like(gru.w.weight)
    from go_slam_amd.droid_net import pack_1x1_weight
    assert torch.equal(gru._ww_pack, pack_1x1_weight(gru.w.weight))


def test_update_module_packs_follow_its_weights():
    from go_slam_amd.droid_net import UpdateModule
    op = UpdateModule()

    def check():
        w, b = op._head_weights()
        assert torch.equal(w, torch.cat([op.delta[0].weight, op.weight[0].weight, op.agg.conv1.weight]).half())
        assert torch.equal(b[2], op.agg.conv1.bias) and op._head_weights()[0] is w
        wpad, bias = op._corr_enc0_padded()
        assert wpad.dtype == torch.float16 and tuple(wpad.shape) == (128, 208) and bias.dtype == torch.float32
        assert torch.equal(wpad[:, :196], op.corr_encoder[0].weight.reshape(128, 196).half())
        assert not wpad[:, 196:].any() and torch.equal(bias, op.corr_encoder[0].bias)
        assert op._corr_enc0_padded()[0] is wpad
    check()
    op.load_state_dict(_fresh_state(op))
    check()
    op.agg.conv1.weight = nn.Parameter(torch.randn_like(op.agg.conv1.weight))       # the merged heads' last member
    op.corr_encoder[0].weight = nn.Parameter(torch.randn_like(op.corr_encoder[0].weight))
    check()
    op.weight[0].bias.data = torch.randn(128)
    op.corr_encoder[0].bias.data = torch.randn(128)
    check()
    op.load_state_dict(_fresh_state(op), assign=True)
    check()


def test_encoder_graph_key_reads_the_live_parameters():
    from go_slam_amd.extractor import BasicEncoder
    enc = BasicEncoder(out_dim=128, norm_fn="instance")
    key = enc._weights_key()
    assert enc._weights_key() == key
    enc.layer3[1].conv2.weight = nn.Parameter(enc.layer3[1].conv2.weight.detach().clone())
    key2 = enc._weights_key()
    assert key2 != key
    enc.load_state_dict(_fresh_state(enc), assign=True)
    key3 = enc._weights_key()
    assert key3 != key2 and enc._weights_key() == key3
    with torch.no_grad():
        enc.conv1.bias.add_(1.0)
        enc.conv2.bias.sub_(1.0)
        enc.conv2.bias.sub_(1.0)
    assert enc._weights_key() != key3


def _fill(op):
    op._head_weights()
    op._corr_enc0_padded()
    op.gru._half_weights()
    return op


def test_copies_start_with_empty_pack_caches():
    from go_slam_amd.droid_net import UpdateModule
    op = _fill(UpdateModule())
    assert op._packs._entries and op.gru._packs._entries
    filled, empty = len(pickle.dumps(op)), len(pickle.dumps(UpdateModule()))
    assert abs(filled - empty) < 4096, (filled, empty)      # the GRU's packs alone are 9 MB
    for dup in (copy.deepcopy(op), pickle.loads(pickle.dumps(op))):
        assert not dup._packs._entries and not dup.gru._packs._entries
        with torch.no_grad():
            dup.agg.conv1.bias.add_(1.0)                    # the copy's own weights, not the original's
        _fill(dup)
        assert torch.equal(dup._head_weights()[1][2], dup.agg.conv1.bias)
        assert not torch.equal(dup._head_weights()[1][2], op._head_weights()[1][2])
        assert dup._packs._entries and dup.gru._packs._entries
