#!/usr/bin/env python3
"""Prediction export of an EgoPack checkpoint (the one main_egopack.py writes): what predict.py exports, from the logits the EgoPack
validation scores, plus what every node retrieved from each auxiliary task's prototype bank -- the prototypes, their distances, their
(verb, noun) labels and how much of the first GraphONE stage's aggregated message each of them supplied.

    python predict_egopack.py enable_graphone=True resume_from=<EgoPack checkpoint> enabled_tasks=[oscc] graphone.k=4 ... predict.out=<dir>

The entry point lives in egopack_amd.predict_egopack; the loops are those of egopack_amd.predict."""
from egopack_amd.predict_egopack import main, predict_egopack_config  # noqa: F401

if __name__ == "__main__":
    main()
