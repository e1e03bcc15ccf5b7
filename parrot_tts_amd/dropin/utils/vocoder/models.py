from parrot_tts_amd.discriminator_train import TrainableMultiPeriodDiscriminator as MultiPeriodDiscriminator  # noqa: F401
from parrot_tts_amd.gan_loss import discriminator_loss, feature_loss, generator_loss  # noqa: F401
from parrot_tts_amd.msd_train import TrainableMultiScaleDiscriminator as MultiScaleDiscriminator  # noqa: F401
from parrot_tts_amd.vocoder import CodeGenerator  # noqa: F401
from parrot_tts_amd.vocoder_train import TrainableCodeGenerator  # noqa: F401
