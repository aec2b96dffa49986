"""Every sub-command's parameters against tests/golden/cli_options.json: name,
option strings, type, default, required, is_flag, help text and position.  The
file pins what `--help` prints and what the command functions receive, option
for option, so a change to how the options are declared cannot move one.

    python tests/test_cli_options.py --write

regenerates the file from the tree's own `main` (only when an option is meant
to change).
"""
import json
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_options.json")


def _plain(v):
    if isinstance(v, (tuple, list)):
        return [_plain(x) for x in v]
    return v if v is None or isinstance(v, (bool, int, float, str)) else repr(v)


def describe(param):
    t = param.type
    return {
        "name": param.name,
        "kind": type(param).__name__,
        "opts": list(param.opts),
        "secondary_opts": list(param.secondary_opts),
        "type": t.name,
        "choices": _plain(getattr(t, "choices", None)),
        "range": [_plain(getattr(t, "min", None)), _plain(getattr(t, "max", None))],
        "file_mode": getattr(t, "mode", None),
        "default": _plain(param.default),
        "required": bool(param.required),
        "is_flag": bool(getattr(param, "is_flag", False)),
        "multiple": bool(param.multiple),
        "nargs": param.nargs,
        "metavar": param.metavar,
        "show_default": _plain(getattr(param, "show_default", None)),
        "help": getattr(param, "help", None),
    }


def table():
    from metacov_amd.cli import main
    return {name: {"help": cmd.help, "params": [describe(p) for p in cmd.params]}
            for name, cmd in sorted(main.commands.items())}


def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


COMMANDS = ("bases", "compare", "consensus", "coverage", "depth", "diversity", "pileup", "scan")


def test_commands():
    assert sorted(table()) == sorted(_golden()) == sorted(COMMANDS)


@pytest.mark.parametrize("command", COMMANDS)
def test_options(command):
    got, want = table()[command], _golden()[command]
    assert got["help"] == want["help"]
    assert [p["name"] for p in got["params"]] == [p["name"] for p in want["params"]]      # the positions
    for g, w in zip(got["params"], want["params"]):
        assert g == w, "%s %s" % (command, w["name"])


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] != ["--write"]:
        raise SystemExit(__doc__)
    with open(GOLDEN, "w") as fh:
        json.dump(table(), fh, indent=1, sort_keys=True)
        fh.write("\n")
