"""image_denoising_amd — MI355X-native Neighbor2Neighbor U-Net training path.

Drop-in for the hot path of lmh9507/image_denoising (arch_unet.UNet, train.py's N2N
sub-sampler, the N2N / Structure losses, Adam) computed by hand-written gfx950 HIP kernels
behind the C-ABI of libdenoise_hip.so (include/denoise_hip.h).
"""
from .adapter import DenoiserWithAdapter, OutputAdapter  # noqa: F401
from .arch_unet import UNet, reference_init  # noqa: F401
from .data import DevicePatchSampler, epoch_plan  # noqa: F401
from .improved_unet import ImprovedUNet  # noqa: F401
from .n2n import (AugmentNoise, generate_mask_pair, generate_subimages,  # noqa: F401
                  n2n_loss, n2n_subsample)
from .resnet import RESNET  # noqa: F401
from .optim import FlatAdam, GradGuard, lr_at_epoch  # noqa: F401
from .trainer import N2NTrainer, StructureTrainer, SupervisedTrainer  # noqa: F401
from .util import L1FFT, Structure_loss  # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):
    # FinetuneTrainer on first use: `python -m image_denoising_amd.finetune` then executes the
    # module once, not a second copy beside one this package already imported
    if name == "FinetuneTrainer":
        from .finetune import FinetuneTrainer

        return FinetuneTrainer
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
