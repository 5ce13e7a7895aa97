"""Kernel resource usage of every MSDeformAttn kernel: tools/kernel_resource_usage.py with the pattern 'msda*.hip' (the old name, kept):

    python tools/msda_resource_usage.py > profiles/msda_resource_usage.txt

With arguments: saved remark files to parse instead of compiling, as before.
The fp32 kernels' lines must not move when a kernel next to them is added or templated."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_resource_usage import FIELDS, listing, parse  # noqa: E402,F401
import kernel_resource_usage  # noqa: E402


def main():
    args = sys.argv[1:]
    kernel_resource_usage.main((["--remarks"] + args) if args else [], default_patterns=("msda*.hip",))


if __name__ == "__main__":
    main()
