"""GPU: pieces.write_pieces with --wav settings against audio.Renderer called directly on the same note lists.  (The four
commands' main() with --wav run in test_render_gpu.py, test_morph_gpu.py and test_latent_edit_gpu.py.)"""
import os

import pytest

pytestmark = pytest.mark.gpu

import melo_gan_amd  # noqa: E402,F401
from melo_gan_amd import audio, pieces  # noqa: E402

from test_pieces_cpu import note_lists, three_pieces  # noqa: E402


def test_write_pieces_wavs_are_the_renderers(tmp_path):
    todo = three_pieces()
    keys = [list(f) for f, _ in todo]
    out, ref = tmp_path / "out", tmp_path / "ref"
    os.makedirs(ref)
    files = pieces.write_pieces(str(out), todo, {"fs": 8000, "voice": "sine", "peak_db": -1.0})
    r = audio.Renderer("cuda", 8000, "sine", -1.0, pieces.WAV_MAX_SECONDS)
    pcm = r.render(note_lists(todo))
    assert len(files) == len(pcm) == 3
    for (f, _), got, k, q, rep in zip(todo, files, keys, pcm, r.report):
        assert got is f and list(got) == k + ["wav", "seconds", "truncated"]
        assert got["wav"] == f["file"][:-4] + ".wav" and (got["seconds"], got["truncated"]) == (rep.seconds, rep.truncated)
        assert rep.seconds > 0 and not rep.truncated
        audio.write_wav(str(ref / got["wav"]), q, 8000)
        assert (out / got["wav"]).read_bytes() == (ref / got["wav"]).read_bytes()
    assert sorted(os.listdir(out)) == sorted([f["file"] for f in files] + [f["wav"] for f in files])
