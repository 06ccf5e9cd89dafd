"""Host-side halves of the captured serving paths: the token check that replaces T5EncoderModel.forward's device-side
range checks for `capture_graph(from_tokens=True)`, the `step_noise` shape check, and the export of the re-noising kernel."""
import pytest
import torch

import abi
import cases
from consistencytta_amd.text_encoder import check_tokens

VOCAB, B, L = cases.TINY_T5["vocab_size"], 2, 8


def _valid():
    ids = torch.tensor([[5, 17, 400, 3, 1, 0, 0, 0], [VOCAB - 1, 1, 0, 0, 0, 0, 0, 0]], dtype=torch.int64)
    mask = torch.tensor([[1, 1, 1, 1, 1, 0, 0, 0], [1, 1, 0, 0, 0, 0, 0, 0]], dtype=torch.int64)
    return ids, mask


def test_token_check_passes_a_valid_batch():
    ids, mask = _valid()
    check_tokens(ids, mask, VOCAB, B, L)
    check_tokens(ids, mask.bool(), VOCAB, B, L)
    one = torch.zeros(B, L, dtype=torch.int64)
    one[:, 0] = 1                                       # rows of a single token (the prompt ""), ids at the range's ends
    check_tokens(torch.tensor([[0] * L, [VOCAB - 1] * L]), one, VOCAB, B, L)


def test_token_check_raises_on_an_id_at_vocab():
    ids, mask = _valid()
    ids[1, 1] = VOCAB
    with pytest.raises(IndexError):
        check_tokens(ids, mask, VOCAB, B, L)


def test_token_check_raises_on_a_negative_id():
    ids, mask = _valid()
    ids[0, 7] = -1                                      # even under padding: the embedding kernel reads every position < L
    with pytest.raises(IndexError):
        check_tokens(ids, mask, VOCAB, B, L)


def test_token_check_raises_on_an_all_padding_row():
    ids, mask = _valid()
    mask[1] = 0
    with pytest.raises(ValueError):
        check_tokens(ids, mask, VOCAB, B, L)


@pytest.mark.parametrize("shape", [(B, L - 1), (B + 1, L), (B * L,)])
def test_token_check_raises_on_a_shape_other_than_the_bucket(shape):
    ids = torch.ones(shape, dtype=torch.int64)
    with pytest.raises(ValueError):
        check_tokens(ids, torch.ones(shape, dtype=torch.int64), VOCAB, B, L)
    good, mask = _valid()
    with pytest.raises(ValueError):
        check_tokens(good, torch.ones(shape, dtype=torch.int64), VOCAB, B, L)


def test_step_noise_with_the_wrong_leading_dimension_raises_before_any_launch():
    """num_steps = 3 re-noises twice: (2, B, C, H, W).  The check runs before the scheduler or an engine is touched, so it
    raises on host tensors (anything later would: there is no CPU path)."""
    from consistencytta_amd import modules
    from consistencytta_amd.models import ConsistencyTTA
    cfg = cases.TINY_UNET
    vae = modules.AutoencoderKL(ddconfig=cases.TINY_VAE_DD, embed_dim=8, scale_factor=0.9, hifigan_config=cases.TINY_HIFIGAN)
    pipe = ConsistencyTTA(unet_config=cfg, vae=vae).eval().requires_grad_(False)
    x, _, _, enc, mask = cases.unet_inputs(cfg, B, 32, 16, 5, "serve_cpu")
    for bad in (torch.zeros((1,) + tuple(x.shape)), torch.zeros((3,) + tuple(x.shape)), torch.zeros_like(x)):
        with pytest.raises(ValueError, match="step_noise"):
            pipe.generate_latent(enc, mask, x, 4.0, 1.0, 3, step_noise=bad)
        with pytest.raises(ValueError, match="step_noise"):
            pipe.forward_from_embeds(enc, mask, x, 4.0, 1.0, 3, step_noise=bad)
    with pytest.raises(ValueError, match="step_noise"):
        pipe.generate_latent(enc, mask, x, 4.0, 1.0, 1, step_noise=torch.zeros((1,) + tuple(x.shape)))


def test_renoise_kernel_is_exported_and_bound():
    abi.assert_bound(("ctta_consistency_renoise",))
