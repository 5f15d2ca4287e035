"""The harness's mode handling, host side (--dry-placement: no GPU call): two different --seamless* options are refused before anything
is looked at, and every mode's report carries its own key and no other mode's."""
import itertools
import json
import subprocess

import pytest

# option -> (its key in the report, the chain options its recipe covers)
MODES = {"--seamless": ("seamless", ()),
         "--seamless-agc": ("seamless_agc", ("--agc-profile", "digital")),
         "--seamless-dc": ("seamless_dc", ("--dc-block",)),
         "--seamless-dc-agc": ("seamless_dc_agc", ("--dc-block", "--agc-profile", "digital")),
         "--seamless-rms": ("seamless_rms", ("--agc-profile", "dx"))}
BASE = ("--synthetic", "2000003", "--synthetic-hash", "7", "--raw-file-input-rate", "2400000", "--raw-file-input-sample-format", "cs16",
        "--output-rate", "744187.5", "--output-sample-format", "cs16", "--freq-shift", "200000", "--shards", "3", "--chunk-frames", "16384",
        "--dry-placement", "--no-numa-bind")


def harness(*args):
    import iq_tool_amd
    from iq_tool_amd.build import HARNESS_BIN
    iq_tool_amd.load()
    return subprocess.run([HARNESS_BIN, *BASE, *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("a,b", list(itertools.combinations(MODES, 2)))
def test_two_seamless_options_exclude_each_other(a, b):
    for first, second in ((a, b), (b, a)):
        # (with the chain options of both, and with an input file that does not exist: refused before either is looked at)
        for extra in ((), ("--dc-block", "--agc-profile", "digital"), ("-i", "/nonexistent/input.cs16")):
            r = harness(first, second, *extra)
            assert r.returncode == 2 and "exclude" in r.stderr and not r.stdout, (first, second, extra, r.returncode, r.stderr)
            assert first in r.stderr and second in r.stderr


@pytest.mark.parametrize("flag", list(MODES))
def test_the_dry_report_carries_the_key_of_its_mode_and_of_no_other(flag):
    key, chain = MODES[flag]
    r = harness(flag, *chain)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout)
    assert info["dry_placement"] is True and info[key] is True
    assert not [k for k, _ in MODES.values() if k != key and k in info]
    assert len(info["per_shard"]) == 3 and all("preroll_frames" in ps for ps in info["per_shard"])
    # the same option twice is one option
    assert harness(flag, flag, *chain).stdout == r.stdout


def test_independent_shards_carry_no_mode_key():
    r = harness()
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout)
    assert not [k for k, _ in MODES.values() if k in info] and "preroll_frames" not in info["per_shard"][0]
