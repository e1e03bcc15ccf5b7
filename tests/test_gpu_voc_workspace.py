"""GPU: every vocoder workspace has ONE layout function that both sizes and carves it (voc_scratch / chunk_scratch, host_voc.hip).
Held here from outside: the size queries return what tests/golden/workspace_bytes.json records (tools/make_workspace_goldens.py, taken
from the library before the layouts were unified; default switches), a raw forward with exactly that many bytes succeeds, and one with
256 bytes (one arena granule) fewer is refused before anything is written."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from parrot_tts_amd import _lib, synth  # noqa: E402
from parrot_tts_amd.ops import dptr, stream_ptr  # noqa: E402
from parrot_tts_amd.vocoder import AttrDict, CodeGenerator  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARROT_OK, PARROT_E_NOMEM = 0, -4

with open(os.path.join(ROOT, "tests", "golden", "workspace_bytes.json")) as _f:
    GOLDEN = json.load(_f)


def _gen(h):
    g = CodeGenerator(AttrDict(h))
    g.load_state_dict(synth.synth_voc_state_dict(h, seed=1234, scale=1.0))
    return g.eval().to(DEV)


@pytest.fixture(scope="module")
def small():
    return _gen(synth.small_voc_config())


# either side of the B x U = 8192 rule: three concurrent MRF branches (3 + 9 activation buffers) up to it, one (3 + 3) above
@pytest.mark.parametrize("B,U", [(1, 40), (8, 1024), (8, 1025), (3, 2731)])
def test_direct_forward_fits_exactly_the_queried_workspace(small, B, U):
    g, lib = small, _lib.lib()
    b = synth.synth_voc_batch(B, U, synth.small_voc_config(), seed=B + U)
    code, spkr = b["code"].to(DEV), b["spkr"].to(DEV).reshape(-1).contiguous()
    want = g(code=code, spkr=spkr)  # the module's own forward (its own workspace)
    hdl = g._current_handle(code.device)
    n = lib.parrot_voc_workspace_bytes(hdl, B, U)
    print(f"voc_workspace_bytes({B}, {U}) = {n}, recorded {GOLDEN['voc_small'][f'{B}x{U}']}")
    assert n == GOLDEN["voc_small"][f"{B}x{U}"]
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    wav = torch.full_like(want, 7.0)
    with torch.cuda.device(code.device):
        rc = lib.parrot_voc_forward(hdl, dptr(code), dptr(spkr), None, B, U, dptr(wav), None, dptr(ws), n, stream_ptr(code.device))
        assert rc == PARROT_OK, lib.parrot_last_error()
        torch.cuda.synchronize()
        assert torch.equal(wav, want)
        wav.fill_(7.0)
        rc = lib.parrot_voc_forward(hdl, dptr(code), dptr(spkr), None, B, U, dptr(wav), None, dptr(ws), n - 256, stream_ptr(code.device))
        assert rc == PARROT_E_NOMEM
        torch.cuda.synchronize()
    assert bool((wav == 7.0).all())


# several lanes | a single chunk (one lane, with the shape's branch streams) | the shape whose trailing chunk once wanted more
# branch streams than its lane was sized for (tests/test_gpu_round4.py)
@pytest.mark.parametrize("cfg,B,U,chunk", [("small", 2, 100, 32), ("small", 2, 20, 32), ("default", 40, 415, 256)])
def test_chunked_forward_fits_exactly_the_queried_workspace(small, cfg, B, U, chunk):
    h = synth.small_voc_config() if cfg == "small" else synth.default_voc_config()
    g, lib = (small if cfg == "small" else _gen(h)), _lib.lib()
    b = synth.synth_voc_batch(B, U, h, seed=B + U)
    code, spkr = b["code"].to(DEV), b["spkr"].to(DEV).reshape(-1).contiguous()
    whole = g(code=code, spkr=spkr)
    hdl = g._current_handle(code.device)
    n = lib.parrot_voc_chunked_workspace_bytes(hdl, B, chunk, -1)
    print(f"voc_chunked_workspace_bytes({cfg}, {B}, {chunk}) = {n}, recorded {GOLDEN['voc_chunked'][f'{cfg}:{B}x{chunk}']}")
    assert n == GOLDEN["voc_chunked"][f"{cfg}:{B}x{chunk}"]
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    wav = torch.empty_like(whole)
    with torch.cuda.device(code.device):
        rc = lib.parrot_voc_forward_chunked(hdl, dptr(code), dptr(spkr), None, B, U, chunk, -1, dptr(wav), dptr(ws), n, stream_ptr(code.device))
    assert rc == PARROT_OK, lib.parrot_last_error()
    torch.cuda.synchronize()
    err = float((wav - whole).abs().max())
    print(f"chunked vs whole: max |diff| = {err:.3e}")
    assert err <= 2e-5  # (the bound of this comparison in tests/test_gpu_round4.py)
