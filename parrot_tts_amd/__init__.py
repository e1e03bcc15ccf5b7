def __getattr__(name):
    # (resolved on first use: importing the package itself loads neither torch nor the HIP library)
    if name == "TrainableCodeGenerator":
        from .vocoder_train import TrainableCodeGenerator
        return TrainableCodeGenerator
    if name == "TrainableMultiPeriodDiscriminator":
        from .discriminator_train import TrainableMultiPeriodDiscriminator
        return TrainableMultiPeriodDiscriminator
    if name == "TrainableMultiScaleDiscriminator":
        from .msd_train import TrainableMultiScaleDiscriminator
        return TrainableMultiScaleDiscriminator
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
