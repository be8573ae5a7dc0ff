"""Train the codec: `python tools/train.py --config PATH` (the package's `train.main`)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from unified_point_cloud_compression_amd.train import main  # noqa: E402

if __name__ == "__main__":
    main()
