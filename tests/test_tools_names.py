"""No file of tools/ bears the name of a standard module: `python tools/X.py` puts tools/ at the front of sys.path, so such a file would
be imported in the standard module's place by every other tool (torch imports `base64` through email.base64mime).  No GPU needed."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_no_tool_shadows_a_standard_module():
    stems = {os.path.splitext(f)[0] for f in os.listdir(os.path.join(ROOT, "tools")) if f.endswith(".py")}
    found_on_the_path = set(sys.stdlib_module_names) - set(sys.builtin_module_names)       # a built-in module is found before sys.path is searched
    assert not stems & found_on_the_path, sorted(stems & found_on_the_path)
