"""CPU checks of how the flat train steps lay a model out (coskad_amd.trainer._FlatStack): which segment kind every layer gets, where
every segment's PReLU-weight gradient goes, and what the step objects expose.  Construction only: no kernel runs (the built library is
needed for the shape queries, as in test_wide_latent_host.py)."""
import pytest
import torch

from coskad_amd import trainer
from coskad_amd.models.sts.ae import STSAE, STSE

DEFAULT = ([32, 16, 32], 64, 8)      # widths, hidden, latent


def _stse(V, widths=DEFAULT[0], hidden=DEFAULT[1], latent=DEFAULT[2], encoder='sts_gcn', projector='linear'):
    torch.manual_seed(0)
    return STSE(2, list(widths), hidden, latent, 12, V, encoder, projector, 'euclidean', 0.0).train()


def _stsae(V, widths=DEFAULT[0], hidden=DEFAULT[1]):
    torch.manual_seed(0)
    return STSAE(2, list(widths), hidden, 8, 12, V, 'sts_gcn', 'linear', 'euclidean', 0.0).train()


def _kinds(stack):
    assert all(s[0] == s.kind for s in stack.segs)       # index 0 reads the kind too
    return [s.kind for s in stack.segs]


def _check_slope_routing(stack, fp, prefix, first=0):
    """segs[k - 1].out_slope_grad is what segment k's backward is handed: None iff segment k - 1 is wide, else the gradient view of the
    PReLU weight of the layer just below segment k; last_slope_grad likewise for the last layer"""
    i = first
    for seg in stack.segs:
        i += len(seg.layers) if seg.kind == 'tile' else 1
        if seg.kind == 'wide':
            assert seg.out_slope_grad is None
        else:
            assert seg.out_slope_grad.data_ptr() == fp.gviews[f"{prefix}{i - 1}.prelu.weight"].data_ptr(), (prefix, i - 1, seg.kind)
    last = stack.segs[-1].out_slope_grad
    assert (stack.last_slope_grad is None) == (last is None)
    assert last is None or stack.last_slope_grad.data_ptr() == last.data_ptr()
    return i


ENCODER_STEPS = [    # V, (widths, hidden, latent), kinds
    (17, DEFAULT, ['tile']),
    (25, DEFAULT, ['tile', 'commute', 'tile']),
    (17, ((64, 128, 256), 256, 16), ['tile', 'wide', 'wide', 'wide']),
    (17, ((32, 128, 16), 64, 8), ['tile', 'wide', 'wide', 'tile']),
]


@pytest.mark.parametrize("V,shape,kinds", ENCODER_STEPS)
def test_encoder_step_segments(V, shape, kinds):
    m = _stse(V, *shape)
    eng = trainer.STSETrainStep(m, lr=0.0)
    assert _kinds(eng.stack) == kinds
    assert _check_slope_routing(eng.stack, eng.fp, "encoder.model.") == len(m.encoder.model)


AE_STEPS = [         # V, widths, hidden, encoder kinds, decoder kinds (behind the folded first layer)
    (17, [32, 16, 32], 64, ['tile'], ['commute', 'tile', 'narrow']),
    (25, [32, 16, 32], 64, ['tile', 'commute', 'tile'], ['commute', 'tile', 'narrow']),
    (17, [16, 32], 32, ['tile'], ['commute', 'narrow']),
    (25, [16, 32], 32, ['tile'], ['commute', 'narrow']),
    (17, [32, 2, 32], 64, ['tile', 'narrow', 'tile'], ['narrow', 'tile', 'narrow']),
    (25, [32, 2, 32], 64, ['tile', 'narrow', 'tile'], ['narrow', 'tile', 'narrow']),
]


@pytest.mark.parametrize("V,widths,hidden,enc,dec", AE_STEPS)
def test_autoencoder_step_segments(V, widths, hidden, enc, dec, monkeypatch):
    m = _stsae(V, widths, hidden)
    eng = trainer.STSAETrainStep(m, mode='ae', lr=0.0)
    assert eng.lowrank is not None
    assert (_kinds(eng.enc), _kinds(eng.dec)) == (enc, dec)
    assert _check_slope_routing(eng.enc, eng.fp, "encoder.model.") == len(m.encoder.model)
    assert _check_slope_routing(eng.dec, eng.fp, "decoder.model.", first=1) == len(m.decoder.model)
    # switched off, the commuted / narrow layers join the neighbouring tile runs
    monkeypatch.setattr(trainer, "COMMUTE", False)
    monkeypatch.setattr(trainer, "NARROW_OUT", False)
    eng = trainer.STSAETrainStep(_stsae(V, widths, hidden), mode='ae', lr=0.0)
    assert (_kinds(eng.enc), _kinds(eng.dec)) == (['tile'], ['tile'])
    assert [len(s.layers) for s in eng.enc.segs + eng.dec.segs] == [len(m.encoder.model), len(m.decoder.model) - 1]
    _check_slope_routing(eng.enc, eng.fp, "encoder.model.")
    _check_slope_routing(eng.dec, eng.fp, "decoder.model.", first=1)


@pytest.mark.parametrize("switch,enc,dec", [("COMMUTE", ['tile'], ['tile', 'narrow']),
                                            ("NARROW_OUT", ['tile', 'commute', 'tile'], ['commute', 'tile'])])
def test_one_switch_off_leaves_the_other_kind(switch, enc, dec, monkeypatch):
    monkeypatch.setattr(trainer, switch, False)
    eng = trainer.STSAETrainStep(_stsae(25), mode='ae', lr=0.0)
    assert (_kinds(eng.enc), _kinds(eng.dec)) == (enc, dec)
    _check_slope_routing(eng.dec, eng.fp, "decoder.model.", first=1)


def test_encoder_step_surface():
    """what bench.py and the Lightning wrapper read off an STSETrainStep"""
    eng = trainer.STSETrainStep(_stse(17), lr=1e-4)
    assert len(eng.layers) == 4 and eng.layers is eng.stack.segs[0].layers
    assert eng.tail_off == eng.fp.offsets["btlnk.weight"] == 30816
    assert eng.world == 1 and eng.steps == 0 and eng.ws is not None
    assert eng.stack.top([None])[1] is eng.layers
    eng.set_lr(3e-4)
    assert eng.lr == 3e-4 and abs(float(eng.hyper[0]) - 3e-4) < 1e-10
    assert trainer.STSETrainStep(_stse(25), lr=0.0).layers == []


def test_plain_chain_when_the_step_asks_for_it():
    """hipGraph capture keeps the 25-joint encoder on the plain chain (one tile run, no commuted segment)"""
    eng = trainer.STSETrainStep(_stse(25), lr=0.0, use_graph=True)
    assert _kinds(eng.stack) == ['tile'] and len(eng.layers) == 4
    with pytest.raises(ValueError, match="wide layers runs on the main stream"):
        trainer.STSETrainStep(_stse(17, (32, 128, 16), 64, 8), lr=0.0, use_graph=True)


def test_make_train_step_choice():
    assert type(trainer.make_train_step(_stse(17), lr=1e-4)) is trainer.STSETrainStep
    assert type(trainer.make_train_step(_stse(17, latent=64), lr=1e-4)) is trainer.STSETrainStep
    assert type(trainer.make_train_step(_stse(17, encoder='learnable_gcn'), lr=1e-4)) is trainer.AutogradTrainStep


# ---- the route is decided at construction --------------------------------------------------------------------------------------------
def _ae(widths, hidden, T=12, V=17, latent=8):
    torch.manual_seed(0)
    return STSAE(2, list(widths), hidden, latent, T, V, 'sts_gcn', 'linear', 'euclidean', 0.0).train()


def _vae(V=17, projector='linear', distribution='ps', latent=8):
    from coskad_amd.models.sts.vae import STSVAE
    torch.manual_seed(0)
    return STSVAE(2, [32, 16, 32], 64, latent, 12, V, 'sts_gcn', projector, 'euclidean', 0.0, distribution=distribution).train()


@pytest.mark.parametrize("widths,hidden,V,which", [([32, 128], 128, 17, "an encoder"), ([128, 32], 64, 17, "a decoder"),
                                                   ([32, 16, 64], 64, 25, "an encoder")])      # (64 -> 64 at 25 joints)
def test_a_stack_ending_wide_is_refused_at_construction(widths, hidden, V, which):
    """a last segment that hands over an activated output: refused by the constructor, before the parameters move into the flat buffer
    and before any kernel (the encoder forward writes BatchNorm running statistics) could run"""
    m = _ae(widths, hidden, V=V)
    ptrs = [p.data_ptr() for p in m.parameters()]
    with pytest.raises(NotImplementedError, match=f"STSAETrainStep: {which} ending in a wide layer"):
        trainer.STSAETrainStep(m, mode='ae')
    assert [p.data_ptr() for p in m.parameters()] == ptrs
    assert trainer.make_decoder_step(m, 'ae') is None


# which (T, V, fused_window) get the flat step; everything else: None (torch autograd + torch.optim.Adam).  The expected column is the
# rule the Lightning wrapper applied while it held this logic (its `is_cuda` half stays there), evaluated per model and written out.
_BOTH = (True, False)
DECODER_STEP = {     # (widths, hidden, latent) -> {(T, V, fused_window)}
    ((32, 16, 32), 64, 8): {(12, V, f) for V in (17, 18, 25) for f in _BOTH} | {(T, V, True) for T in (8, 16, 24) for V in (17, 25)},
    ((16, 8, 16), 16, 8): {(12, V, f) for V in (17, 18, 25) for f in _BOTH},            # 8-channel layers: no window kernels
    ((32, 128), 128, 8): set(),                                                          # the encoder ends wide
    ((128, 32), 64, 8): set(),                                                           # the decoder ends wide
    ((32, 16, 64), 64, 8): {(12, V, f) for V in (17, 18) for f in _BOTH},                # ... at 25 joints
    ((32, 16, 32), 64, 32): set(),                                                       # latent beyond the bottleneck kernels
}


@pytest.mark.parametrize("shape", list(DECODER_STEP), ids=lambda s: "-".join(map(str, s[0])) + f"-h{s[1]}-l{s[2]}")
def test_decoder_step_decision_table(shape):
    (widths, hidden, latent), steps = shape, DECODER_STEP[shape]
    for T in (8, 12, 16, 24):
        for V in (17, 18, 25):
            for fused in _BOTH:
                eng = trainer.make_decoder_step(_ae(widths, hidden, T, V, latent), 'ae', fused_window=fused, lr=0.0)
                assert (eng is not None) == ((T, V, fused) in steps), (T, V, fused)
                if eng is not None:      # a step at a window length is the fused one, cut without a `wide` segment
                    assert type(eng) is trainer.STSAETrainStep
                    assert ('window' in _kinds(eng.enc)) == (T != 12) and 'wide' not in _kinds(eng.enc) + _kinds(eng.dec)


def test_encoder_step_projector_forms():
    lin, mlp = trainer.STSETrainStep(_stse(17), lr=0.0), trainer.STSETrainStep(_stse(17, projector='mlp'), lr=0.0)
    assert type(lin.projector) is trainer._LinearProjector and type(mlp.projector) is trainer._MLPProjector
    assert lin.projector.gW is lin.fp.gviews["btlnk.weight"] and lin.projector.gb is lin.fp.gviews["btlnk.bias"]
    assert mlp.projector.gW is mlp.fp.gviews["btlnk.net.0.weight"] and mlp.projector.lin is mlp.model.btlnk.net[0]
    assert [g["W2"] for _, _, g in mlp.projector.blocks] == [mlp.fp.gviews["btlnk.net.3.weight"]]


DECODER_STAGES = [   # model, mode, projector form, latent form, the latent head applies the two small heads
    (lambda: _ae([32, 16, 32], 64), 'ae', "_LinearProjector", "_CentreLatent", False),
    (lambda: _vae(17), 'vae', "_StackedHeads", "_PowerSphericalLatent", False),
    (lambda: _vae(25, projector='mlp'), 'vae', "_MLPProjector", "_PowerSphericalLatent", True),
    (lambda: _vae(17, distribution='normal'), 'vae', "_StackedHeads", "_AutogradLatent", False),
    (lambda: _vae(17, projector='mlp', distribution='normal'), 'vae', "_MLPProjector", "_AutogradLatent", True),
]


@pytest.mark.parametrize("build,mode,projector,latent,heads", DECODER_STAGES, ids=[f"{r[2]}-{r[3]}" for r in DECODER_STAGES])
def test_decoder_step_stage_forms(build, mode, projector, latent, heads, monkeypatch):
    from coskad_amd import lowrank
    assert trainer.STSAETrainStep.supports(build())
    eng = trainer.STSAETrainStep(build(), mode=mode, lr=0.0)
    assert type(eng.projector) is getattr(trainer, projector) and type(eng.latent) is getattr(trainer, latent)
    assert eng.latent.heads is heads and len(getattr(eng.latent, "head_params", [None] * 4 * heads)) == 4 * heads
    # folded entry: the first decoder layer hands its pre-activation and slope to the stack behind it
    gv = eng.fp.gviews
    assert eng.entry is eng.lowrank and type(eng.lowrank) is lowrank.LowRankFirstLayer
    assert eng.entry_slope is eng.model.decoder.model[0].prelu.weight and eng.entry_slope_grad is gv["decoder.model.0.prelu.weight"]
    # plain entry: rev_btlnk alone, the stack takes every decoder layer
    monkeypatch.setattr(lowrank, "MODE", "never")
    eng = trainer.STSAETrainStep(build(), mode=mode, lr=0.0)
    assert eng.lowrank is None and type(eng.entry) is trainer._PlainEntry
    assert eng.entry_slope is None and eng.entry_slope_grad is None
    assert sum(len(s.layers) if s.kind == 'tile' else 1 for s in eng.dec.segs) == len(eng.model.decoder.model)
    assert eng.entry.gW is eng.fp.gviews["rev_btlnk.weight"]
