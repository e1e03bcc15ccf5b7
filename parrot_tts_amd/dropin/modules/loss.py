from parrot_tts_amd.loss import ModelLoss  # noqa: F401  (reference modules/loss.py)
