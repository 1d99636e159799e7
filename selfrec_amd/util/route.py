"""The engine's route switches: which of two implementations a model takes (a kernel or torch's expression, one stacked
pass or three)."""
import os


def route(env, key, conf, choices=('hip', 'torch')):
    """the environment variable ``env``, else the conf's ``key``, else choices[0]; lower-cased and stripped, and a
    ValueError for anything outside ``choices``"""
    value = os.environ.get(env)
    if value is None and conf is not None and conf.contain(key):
        value = conf[key]
    value = choices[0] if value is None else str(value).strip().lower()
    if value not in choices:
        raise ValueError(f"{key} / {env}: {value!r} is none of {', '.join(repr(c) for c in choices)}")
    return value
