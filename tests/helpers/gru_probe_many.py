"""tests/helpers/gru_probe.py for several shapes in ONE process (the library is chosen at import time, so a comparison of
two builds costs two processes however many shapes it takes): gru_probe_many.py B,W,S [B,W,S ...] prints gru_probe's JSON
line once per shape, in order."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gru_probe  # noqa: E402

if __name__ == "__main__":
    for shape in sys.argv[1:]:
        sys.argv = [sys.argv[0]] + shape.split(",")
        gru_probe.main()
