"""What the streaming API accepts (h264r_picture_begin / h264r_mb_submit / h264r_picture_end_async),
checked without a GPU: oracle/stage_check.cc drives PictureStage of arrow-h264_amd/csrc/picture_stage.h --
the one statement of those checks, shared by libh264r.so and the CPU implementation of the ABI -- on
pictures of 1 x 1 and 2 x 2 MBs and compares every status, and which check wins, with the library's."""
import os
import subprocess

import _oracle as O

STAGE_CHECK = os.path.join(O.ORACLE_DIR, "_cpu", "stage_check")


def test_picture_stage_statuses():
    O.build_oracle()
    r = subprocess.run([STAGE_CHECK], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("stage_check: ok")
