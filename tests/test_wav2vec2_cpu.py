"""CPU checks of the wav2vec 2.0 path: the tests' oracle against ``transformers`` (random weights, built offline), the frame-count
formula, ``Wav2Vec2Weights.from_state_dict`` on the host, and the ABI of the new entry points."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import wav2vec2_oracle as WO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ('mts_w2v_wave_stats', 'mts_w2v_conv0_stats', 'mts_w2v_conv0', 'mts_w2v_regroup', 'mts_w2v_rows', 'mts_w2v_pos_conv')


def _hf_model(cfg):
    tr = pytest.importorskip('transformers')
    hc = tr.Wav2Vec2Config(hidden_size=cfg['hidden'], num_hidden_layers=cfg['layers'], num_attention_heads=cfg['heads'],
                           intermediate_size=cfg['intermediate'], conv_dim=(cfg['conv_dim'],) * len(cfg['kernels']), conv_kernel=cfg['kernels'],
                           conv_stride=cfg['strides'], num_conv_pos_embeddings=cfg['pos_kernel'], num_conv_pos_embedding_groups=cfg['pos_groups'],
                           feat_extract_norm='group', conv_bias=False, do_stable_layer_norm=False, hidden_dropout=0.0, activation_dropout=0.0,
                           attention_dropout=0.0, feat_proj_dropout=0.0, final_dropout=0.0, layerdrop=0.0, mask_time_prob=0.0, mask_feature_prob=0.0,
                           layer_norm_eps=cfg['eps'])
    torch.manual_seed(5)
    return tr, tr.Wav2Vec2Model(hc).eval().double()


def _normalised(tr, x):
    """the processor's normalisation of a raw segment: its formula in fp64.  Wav2Vec2FeatureExtractor, where it constructs without files,
    returns the same numbers rounded to fp32 (it casts its output), which is checked here; the model is fed the unrounded ones so that
    the comparison with the fp64 oracle sees the summation order alone."""
    x = x.double()
    formula = (x - x.mean()) / torch.sqrt(x.var(unbiased=False) + 1e-7)
    try:
        fe = tr.Wav2Vec2FeatureExtractor(feature_size=1, sampling_rate=16000, padding_value=0.0, do_normalize=True, return_attention_mask=False)
    except Exception:  # noqa: BLE001
        return formula
    got = torch.from_numpy(np.asarray(fe(x.numpy(), sampling_rate=16000)['input_values'][0])).double()
    assert float((got - formula).abs().max()) <= 2.0 ** -23 * float(formula.abs().max())
    return formula


@pytest.mark.parametrize('name,n', [('small', 4001), ('base', 24000)])
def test_oracle_equals_transformers(name, n):
    cfg = WO.SMALL if name == 'small' else WO.BASE
    tr, model = _hf_model(cfg)
    x = WO.signals([n], seed=11, offset_at=0)[0]
    with torch.no_grad():
        want = model(_normalised(tr, x)[None]).last_hidden_state[0]
        got = WO.Oracle(model.state_dict(), cfg, 'fp64').forward(x.double())
    assert got.shape == want.shape == (WO.frame_count(n, cfg), cfg['hidden'])
    # the extractor normalises in fp32 when it is handed fp32; here both sides see fp64 samples, so only the summation order differs
    err, scale = float((got - want).abs().max()), float(want.abs().max())
    print(f'{name}: max abs difference {err:.3e}, max |value| {scale:.3e}')
    assert err <= 1e-9 * scale


def test_frame_count_formula_equals_the_model():
    from multimodaltopicsegmentation_amd import wav2vec2 as W
    # 49 999 samples give 155 frames by T <- (T - k) // stride + 1 (9998, 4998, 2498, 1248, 623, 311, 155) and by the model below; 156 is
    # what 50 000 give, which is checked as well
    ns = [400, 719, 720, 16000, 49999, 50000]
    assert [WO.frame_count(n) for n in ns] == [1, 1, 2, 49, 155, 156]
    assert W.frame_counts(ns + [399, 5], WO.BASE['kernels'], WO.BASE['strides']).tolist() == [1, 1, 2, 49, 155, 156, 0, 0]
    tr, model = _hf_model(WO.SMALL)                       # the small size has the base size's kernels and strides
    for n in ns:
        with torch.no_grad():
            assert model.feature_extractor(torch.zeros(1, n, dtype=torch.float64)).shape[2] == WO.frame_count(n)
        assert int(model._get_feat_extract_output_lengths(n)) == WO.frame_count(n)


def _weights(sd, cfg=WO.SMALL, **kw):
    from multimodaltopicsegmentation_amd import Wav2Vec2Weights
    return Wav2Vec2Weights.from_state_dict(sd, WO.hf_config_dict(cfg), device='cpu', **kw)


def test_from_state_dict_spellings_prefix_and_round_trip():
    cfg = WO.SMALL
    a = _weights(WO.random_state_dict(cfg, 3, 'weight_g'), dtype='fp32')
    b = _weights({'wav2vec2.' + k: v for k, v in WO.random_state_dict(cfg, 3, 'parametrizations').items()}, dtype='fp32')
    assert torch.equal(a.pos_w, b.pos_w) and torch.equal(a.proj_w, b.proj_w) and torch.equal(a.layers[1]['qkv_w'], b.layers[1]['qkv_w'])
    assert (a.conv_dim, a.hidden_size, a.intermediate_size, a.num_layers, a.num_heads, a.pos_kernel, a.pos_groups) == (32, 128, 256, 2, 4, 16, 4)
    assert a.kernels == cfg['kernels'] and a.strides == cfg['strides'] and a.min_samples == 400
    # the effective weight is g * v / ||v|| over dims (0, 1), formed in fp64 and rounded once
    ora = WO.Oracle(WO.random_state_dict(cfg, 3), cfg).sd['encoder.pos_conv_embed.conv.weight']          # fp64 [H, H / G, K_p]
    H, G, Kp = cfg['hidden'], cfg['pos_groups'], cfg['pos_kernel']
    assert torch.equal(a.pos_w, ora.permute(0, 2, 1).reshape(G, H // G, Kp * (H // G)).float())
    # extra keys are ignored; the state dict round-trips
    sd = WO.random_state_dict(cfg, 3)
    sd.update({'lm_head.weight': torch.zeros(4, H), 'lm_head.bias': torch.zeros(4), 'quantizer.codevectors': torch.zeros(1, 8, 4),
               'adapter.layers.0.conv.weight': torch.zeros(4, 4, 3), 'project_q.weight': torch.zeros(4, 4)})
    c = _weights(sd, dtype='bf16')
    assert c.pos_w.dtype == torch.bfloat16 and c.conv0_w.dtype == torch.float32 and torch.equal(c.pos_w, a.pos_w.to(torch.bfloat16))
    back = c.state_dict()
    assert not any(k.startswith(('lm_head', 'quantizer', 'adapter', 'project_q', 'masked_spec_embed')) for k in back)
    d = _weights(back, dtype='bf16')
    assert torch.equal(d.pos_w, c.pos_w) and torch.equal(d.layers[0]['ff1_w'], c.layers[0]['ff1_w']) and torch.equal(d.conv_w[4], c.conv_w[4])
    assert set(back) == set(d.state_dict()) and all(torch.equal(back[k], d.state_dict()[k]) for k in back)
    # q | k | v are concatenated in that order
    base = WO.random_state_dict(cfg, 3)
    assert torch.equal(a.layers[0]['qkv_w'][H:2 * H], base['encoder.layers.0.attention.k_proj.weight'])
    assert torch.equal(a.layers[0]['qkv_b'][2 * H:], base['encoder.layers.0.attention.v_proj.bias'])


def test_from_state_dict_refuses_what_it_does_not_cover():
    cfg = WO.SMALL
    sd = WO.random_state_dict(cfg, 4)
    with pytest.raises(NotImplementedError, match='conv_bias=True'):
        _weights({**sd, 'feature_extractor.conv_layers.2.conv.bias': torch.zeros(cfg['conv_dim'])})
    with pytest.raises(NotImplementedError, match="feat_extract_norm='layer'"):
        _weights({**sd, 'feature_extractor.conv_layers.1.layer_norm.weight': torch.ones(cfg['conv_dim']),
                  'feature_extractor.conv_layers.1.layer_norm.bias': torch.zeros(cfg['conv_dim'])})
    odd = dict(sd)
    odd['encoder.pos_conv_embed.conv.weight_v'] = sd['encoder.pos_conv_embed.conv.weight_v'][:, :, :15].contiguous()
    odd['encoder.pos_conv_embed.conv.weight_g'] = sd['encoder.pos_conv_embed.conv.weight_g'][:, :, :15].contiguous()
    with pytest.raises(NotImplementedError, match=r'odd positional kernel \(15\)'):
        _weights(odd)
    from multimodaltopicsegmentation_amd import Wav2Vec2Weights
    with pytest.raises(NotImplementedError, match='do_stable_layer_norm=True'):
        Wav2Vec2Weights.from_state_dict(sd, {**WO.hf_config_dict(cfg), 'do_stable_layer_norm': True})
    with pytest.raises(NotImplementedError, match="hidden_act='relu'"):
        Wav2Vec2Weights.from_state_dict(sd, {**WO.hf_config_dict(cfg), 'hidden_act': 'relu'})
    with pytest.raises(NotImplementedError, match='stride 2'):
        Wav2Vec2Weights.from_state_dict(sd, {**WO.hf_config_dict(cfg), 'conv_stride': (5, 2, 2, 3, 2, 2, 2)})
    with pytest.raises(ValueError, match="'bf16' or 'fp32'"):
        _weights(sd, dtype='fp16')


def test_permuted_conv_weights_reproduce_conv1d_through_overlapping_rows():
    """the layout the device relies on, in NumPy: output row t of a stride-2, kernel-k layer is the product of the overlapping row
    x + 2 t C (row stride 2 C, K = k C) with the weights permuted to [C_out, k * C_in]; the grouped positional convolution likewise per
    group on rows padded with K_p / 2 zeros (row stride H / G, K = K_p H / G)"""
    cfg = WO.SMALL
    sd = WO.random_state_dict(cfg, 6)
    w = _weights(sd, dtype='fp32')
    C, T = cfg['conv_dim'], 23
    x = torch.randn(T, C, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    for layer in (1, 5):
        k = cfg['kernels'][layer]
        want = F.conv1d(x.t()[None], sd[f'feature_extractor.conv_layers.{layer}.conv.weight'].double(), stride=2)[0].t()
        rows = np.lib.stride_tricks.as_strided(x.numpy(), shape=(want.shape[0], k * C), strides=(2 * C * 8, 8))
        got = rows @ w.conv_w[layer - 1].double().numpy().T
        assert np.abs(got - want.numpy()).max() < 1e-12
    H, G, Kp = cfg['hidden'], cfg['pos_groups'], cfg['pos_kernel']
    cg = H // G
    h = torch.randn(T, H, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    ora = WO.Oracle(sd, cfg)
    want = F.conv1d(h.t()[None], ora.sd['encoder.pos_conv_embed.conv.weight'], None, padding=Kp // 2, groups=G)[0][:, :-1].t()
    for g in range(G):
        padded = np.zeros((T + Kp, cg))
        padded[Kp // 2:Kp // 2 + T] = h[:, g * cg:(g + 1) * cg].numpy()
        rows = np.lib.stride_tricks.as_strided(padded, shape=(T, Kp * cg), strides=(cg * 8, 8))
        got = rows @ w.pos_w[g].double().numpy().T
        assert np.abs(got - want[:, g * cg:(g + 1) * cg].numpy()).max() < 1e-6          # the fp32 rounding of the effective weight


def test_new_entry_points_are_declared_bound_and_documented():
    from multimodaltopicsegmentation_amd import _lib as L
    from tests.test_abi import _declared
    decl = _declared()
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    for name in NEW_ENTRY_POINTS:
        assert name in decl, f'{name} is not declared in include/mts.h'
        assert hasattr(L.lib, name) and len(L.SIGNATURES[name][1]) == decl[name], name
        assert re.search(r'`' + name + r'`', doc), f'{name} is missing from INTEGRATION.md'
    # argument validation happens before any device work: safe without a GPU
    assert L.lib.mts_w2v_wave_stats(None, 0, None, 1, None, None, None) == 1
    assert L.lib.mts_w2v_wave_stats(None, 1, None, 1, None, None, None) == 1
    p = 4096                                                        # stands for a device address: never dereferenced by a refused call
    assert L.lib.mts_w2v_conv0_stats(None, 1, 12, 10, 5, p, 100, p, p, p, p, 1e-5, p, p) == 2          # C % 8
    assert L.lib.mts_w2v_conv0_stats(None, 1, 16, 33, 5, p, 100, p, p, p, p, 1e-5, p, p) == 2          # kernel > 32
    assert L.lib.mts_w2v_conv0_stats(None, 1, 16, 10, 0, p, 100, p, p, p, p, 1e-5, p, p) == 1          # stride < 1
    assert L.lib.mts_w2v_conv0(None, 0, 1, 16, 10, 5, p, 100, p, p, p, p, p, p, p, p, p, 100, p) == 1   # rows no multiple of 64
    assert L.lib.mts_w2v_conv0(None, 7, 1, 16, 10, 5, p, 100, p, p, p, p, p, p, p, p, p, 128, p) == 1   # dtype
    assert L.lib.mts_w2v_conv0(None, 0, 1, 16, 10, 5, p, 100, p, p, p, p, p, p, p, p, None, 128, p) == 1
    assert L.lib.mts_w2v_regroup(None, 0, 1, 128, 4, 15, p, p, p, 64, p) == 2                           # odd K_p
    assert L.lib.mts_w2v_regroup(None, 0, 1, 128, 4, 130, p, p, p, 64, p) == 2                          # K_p > 128
    assert L.lib.mts_w2v_regroup(None, 0, 1, 48, 4, 16, p, p, p, 64, p) == 2                            # H / G % 8
    assert L.lib.mts_w2v_regroup(None, 0, 1, 130, 4, 16, p, p, p, 64, p) == 1                           # H % G
    assert L.lib.mts_w2v_regroup(None, 0, 1, 128, 4, 16, p, None, p, 64, p) == 1
    assert L.lib.mts_w2v_rows(None, 0, 1, 1, 6, p, p, None, None, p, 4, p) == 1                         # D % 4
    assert L.lib.mts_w2v_rows(None, 0, 1, 1, 8, p, p, p, None, p, 4, p) == 1                            # res without res_row0
    assert L.lib.mts_w2v_rows(None, 0, 1, 1, 8, p, p, None, None, p, 0, p) == 1
    assert L.lib.mts_w2v_pos_conv(None, 1, 128, 4, 16, p, p, p, p, 0, p, p, p) == 1                     # n_tiles < 1
    assert L.lib.mts_w2v_pos_conv(None, 1, 1024, 8, 16, p, p, p, p, 1, p, p, p) == 2                    # H / G > 64
    assert L.lib.mts_w2v_pos_conv(None, 1, 64, 8, 2, p, p, p, p, 1, p, p, p) == 2                       # K_p * H / G % 128
    assert L.lib.mts_w2v_pos_conv(None, 1, 128, 4, 16, p, p, p, None, 1, p, p, p) == 1


def test_resident_audio_refusals_on_the_host():
    from multimodaltopicsegmentation_amd import ResidentAudio
    w = _weights(WO.random_state_dict(WO.SMALL, 1))
    wave = [np.zeros(3000, dtype=np.float32), np.zeros(3000, dtype=np.float32)]
    with pytest.raises(ValueError, match='fewer than the 4096'):                                        # the default rule stays
        ResidentAudio(wave, [[(0, 1000)], [(0, 1000)]], 'cpu', unit='samples')
    with pytest.raises(ValueError, match='sentence 1 of document 0 has 300 samples, fewer than min_samples = 400'):
        ResidentAudio(wave, [[(0, 1000), (1000, 1300)], [(0, 1000)]], 'cpu', unit='samples', min_samples=400)
    audio = ResidentAudio(wave, [[(0, 1000)], [(0, 500), (500, 899)]], 'cpu', unit='samples', min_samples=1)
    with pytest.raises(ValueError, match=r"sentence 1 of document 1 has 399 samples, fewer than the 400 that give one wav2vec 2.0 frame.*Conv1d raises"):
        audio.wav2vec2(w)
    with pytest.raises(ValueError, match='sentence 0 of document 0 has 1000 samples.*librosa'):
        audio.mfcc()
    ok = ResidentAudio(wave, [[(0, 1000)], [(0, 500)]], 'cpu', unit='samples', min_samples=400)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ok.wav2vec2(w)
    with pytest.raises(ValueError, match="'delta_gap' reads the next sentence's first frame.*wav2vec2\\(weights\\).pool"):
        ok.wav2vec2_stats(w, 'delta_gap')
    with pytest.raises(ValueError, match='Wav2Vec2Weights'):
        ok.wav2vec2({})
