from egopack_amd.graphone import bank_labels, build_graphone  # noqa: F401
