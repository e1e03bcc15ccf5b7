from parrot_tts_amd.aligner import extract_durations_with_dijkstra  # noqa: F401
