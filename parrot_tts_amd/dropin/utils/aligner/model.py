from parrot_tts_amd.aligner import Aligner  # noqa: F401
