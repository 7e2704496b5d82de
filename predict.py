#!/usr/bin/env python3
"""Prediction export of a trained checkpoint: top-k verbs and nouns per node (AR, LTA), the K x Z sampled LTA futures, a
state-change probability per OSCC clip and a key frame per PNR clip, as ``predictions_<task>.pt`` / ``.json``.

    python predict.py resume_from=<checkpoint> enabled_tasks=[ar,lta,oscc,pnr] predict.split=validation predict.topk=5 predict.out=<dir>

The loops and the entry point live in egopack_amd.predict."""
from egopack_amd.predict import main, predict_config, predict_heads, predict_lta, predict_oscc, predict_pnr, to_json  # noqa: F401

if __name__ == "__main__":
    main()
