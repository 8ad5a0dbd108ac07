"""TEST-ONLY: run a call under another BOGP_CHUNK_MB (the sweeps read it per call) and put the environment back."""
import os


def with_chunk_mb(mb, fn):
    old = os.environ.get("BOGP_CHUNK_MB")
    os.environ["BOGP_CHUNK_MB"] = str(mb)
    try:
        return fn()
    finally:
        if old is None:
            del os.environ["BOGP_CHUNK_MB"]
        else:
            os.environ["BOGP_CHUNK_MB"] = old
