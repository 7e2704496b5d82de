#!/usr/bin/env python3
"""Temperature calibration of a trained checkpoint: one validation pass, the fit on the device, ``calibration_<task>.pt`` beside the
checkpoint (predict.py / predict_egopack.py then export the calibrated probabilities of the raw top-k order).

    python calibrate.py resume_from=<checkpoint> enabled_tasks=[ar,lta,oscc]
    python calibrate.py enable_graphone=True resume_from=<EgoPack checkpoint> enabled_tasks=[oscc]

The loop and the entry point live in egopack_amd.calibrate."""
from egopack_amd.calibrate import calibrate_tasks, main  # noqa: F401

if __name__ == "__main__":
    main()
