"""MI355X-native VQ-VAE-2 stage-1 hot path (drop-in for the reference's vqvae.py).

Import as ``vqvae2_amd`` (see /vqvae2_amd.py: the directory name carries hyphens).
Public surface mirrors /root/reference/vqvae.py and distributed/__init__.py:1-13.
"""
from .vqvae import VQVAE, Quantize, ResBlock, Encoder, Decoder, Conv2d, ConvTranspose2d, ReLU  # noqa: F401
from . import vqvae_deep  # noqa: F401
from .vqvae_deep import VQVAE_Deep  # noqa: F401
from . import pixelsnail  # noqa: F401
from .pixelsnail import (CausalAttention, WNConv2d, CausalConv2d, GatedResBlock, PixelBlock, CondResNet,  # noqa: F401
                         PixelSNAIL, set_conv_precision, conv_precision, set_attention_precision, attention_precision)
from .ops import prior_loss, vq_restart_candidates, vq_ema_update_restart  # noqa: F401
from . import distributed  # noqa: F401
from . import ops  # noqa: F401
from . import codes  # noqa: F401
from .optim import FusedAdam, CycleScheduler  # noqa: F401
from .train import Stage1Trainer, Stage2Trainer, stage1_loss  # noqa: F401
from .data import ImageNormalizer, ImageDenormalizer, HostBatchPrefetcher, grid_layout, save_u8_image  # noqa: F401
from .evaluate import Evaluator, PriorEvaluator, score_codes, score_codes_labelled, perplexity_from_counts, psnr_from_mse_u8  # noqa: F401
from . import sample  # noqa: F401
from .sample import PriorSampler, sample_model, load_model  # noqa: F401
