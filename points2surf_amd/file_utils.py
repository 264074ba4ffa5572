"""Host-side file helpers shared by the package and the drop-in (no torch, no device)."""
import os


def call_necessary(files_in, files_out):
    """file_utils.call_necessary (reference source/base/file_utils.py:194-240): inputs exist and an output is missing or
    older"""
    if any(not os.path.isfile(f) for f in files_in):
        print('WARNING: Input file are missing: {}'.format([f for f in files_in if not os.path.isfile(f)]))
        return False
    if any(not os.path.isfile(f) or os.path.getsize(f) == 0 for f in files_out):
        return True
    return max(os.path.getmtime(f) for f in files_in) >= min(os.path.getmtime(f) for f in files_out)
