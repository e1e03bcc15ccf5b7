"""The fused ResBlock kernels after packed-fp32 arithmetic left their operand conversion, and the branch mean without the division
sequence (csrc/div_uniform.h): same results as the layer-by-layer path, and the mean's bits are those of (a + b + c) / 3.

Shapes: the smallest at which every fused kernel still sees an interior window and both edge windows (one window plus a
remainder): 404 columns at 64 channels (window 192), 808 at 32 (384), 1616 at 16 (768); B = 2, one row ragged."""
import pytest
import torch

from parrot_tts_amd import ops, synth
from parrot_tts_amd.vocoder import AttrDict, CodeGenerator

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gen(h, sd):
    g = CodeGenerator(AttrDict(h))
    g.load_state_dict(sd)
    return g.eval().to(DEV)


@pytest.fixture
def precision(request):
    ops.set_default_precision(ops.PREC_NAMES[request.param])
    yield request.param
    ops.set_default_precision(ops.PREC_DEFAULT)


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6"], indirect=True)
def test_fused_path_matches_layer_by_layer(precision):
    """16-, 32- and 64-channel ResBlock1 stages with k = 3, 7, 11 through the fused kernels against PARROT_FUSED=0 (every ResBlock
    layer by layer), under the bound tests/test_gpu_parity.py holds both of them to against the oracle: 5e-5 on the waveform."""
    h = synth.small_voc_config()
    h.update(upsample_initial_channel=128, upsample_rates=[4, 2, 2], upsample_kernel_sizes=[8, 4, 4])
    sd = synth.synth_voc_state_dict(h, seed=21, scale=1.0)
    batch = synth.synth_voc_batch(2, 101, h, seed=9)
    code, spkr = batch["code"].to(DEV), batch["spkr"].to(DEV)
    lens = torch.tensor([101, 77], dtype=torch.int32, device=DEV)
    out = {}
    try:
        for mode in (2, 0):
            ops.set_fused_resblocks(mode)
            stages = {}
            with torch.no_grad():
                y = _gen(h, sd)(code=code, spkr=spkr, unit_lens=lens, stages=stages)
            out[mode] = (y.cpu(), {k: v.cpu() for k, v in stages.items()})
    finally:
        ops.set_fused_resblocks(2)
    hop = 16
    (y1, s1), (y0, s0) = out[2], out[0]
    assert [s1[f"mrf{i}"].shape[1:] for i in range(3)] == [(64, 404), (32, 808), (16, 1616)]
    for b, n in enumerate((101, 77)):  # (samples past a row's end are unspecified)
        err = float((y1[b, :, : n * hop] - y0[b, :, : n * hop]).abs().max())
        print(precision, "row", b, "waveform max abs diff fused vs layer by layer", err)
        assert torch.isfinite(y1[b, :, : n * hop]).all()
        assert err <= 5e-5


def _single_branch(h, sd, j):
    """The generator that keeps ResBlock branch j of a one-stage generator alone (no branch mean: EPI_STORE)."""
    h1 = dict(h, resblock_kernel_sizes=[h["resblock_kernel_sizes"][j]], resblock_dilation_sizes=[h["resblock_dilation_sizes"][j]])
    sd1 = {}
    for k, v in sd.items():
        if not k.startswith("resblocks."):
            sd1[k] = v
        elif k.startswith(f"resblocks.{j}."):
            sd1["resblocks.0." + k.split(".", 2)[2]] = v
    return h1, sd1


# (channels of the MRF stage, batch, units): the pair kernels' per-branch launches with their EPI_STORE / EPI_ADD / EPI_ADD_DIV
# epilogues at 16 / 32 / 64 channels (64 channels, k = 11: the layer kernels' epilogue), and the whole-MRF launch, which takes a
# 32-channel stage of at least two windows per CU (8 rows x 65 windows of 648 columns)
@pytest.mark.parametrize("ch,B,U", [(16, 2, 808), (32, 2, 404), (64, 2, 202), (32, 8, 21000)], ids=["c16", "c32", "c64", "c32_whole_mrf"])
def test_branch_mean_has_the_bits_of_the_division(ch, B, U):
    """xs = (rb_0(x) + rb_1(x) + rb_2(x)) / 3 (models.py:100-106) of a one-stage generator against the three branches taken from
    single-branch generators with the same weights, summed in branch order and divided in torch fp32 on the host: bit for bit."""
    h = synth.small_voc_config()
    h.update(upsample_initial_channel=2 * ch, upsample_rates=[2], upsample_kernel_sizes=[4])
    sd = synth.synth_voc_state_dict(h, seed=33, scale=1.0)
    batch = synth.synth_voc_batch(B, U, h, seed=B + U)
    code, spkr = batch["code"].to(DEV), batch["spkr"].to(DEV)
    lens = torch.full((B,), U, dtype=torch.int32, device=DEV)
    lens[-1] = (3 * U) // 4  # one ragged row
    T = 2 * U

    def mrf0(hh, ss):
        stages = {}
        with torch.no_grad():
            _gen(hh, ss)(code=code, spkr=spkr, unit_lens=lens, stages=stages)
        torch.cuda.synchronize()
        return stages["ups0"].cpu(), stages["mrf0"].cpu()

    x3, got = mrf0(h, sd)
    assert got.shape == (B, ch, T)
    acc = None
    for j in range(3):
        xj, bj = mrf0(*_single_branch(h, sd, j))
        assert torch.equal(xj, x3)  # the same stage input
        acc = bj if acc is None else acc + bj
    want = acc / 3.0
    n_last = 2 * int(lens[-1])
    valid = torch.ones(B, 1, T, dtype=torch.bool)
    valid[-1, :, n_last:] = False  # (columns past a row's end are unspecified)
    valid = valid.expand_as(got)
    assert torch.isfinite(got[valid]).all() and float(got[valid].abs().max()) > 1e-3
    n_diff = int((got.view(torch.int32)[valid] != want.view(torch.int32)[valid]).sum())
    print(ch, B, U, "elements compared", int(valid.sum()), "differing bit patterns", n_diff)
    assert n_diff == 0
