"""CPU tests of the order search's candidate-set tables: their arithmetic on the host
(bin/order_tables_check, plain and under ASan + UBSan: ranks, indices and the serial
butterfly against the list scan), the new export and `ordersearch --tables`' parsing."""
import os
import subprocess

import pytest

import ulg
from test_order_search_ref import PKG


@pytest.mark.parametrize("path", ["bin/order_tables_check", "bin/san/order_tables_check"])
def test_order_tables_check(path):
    if not os.path.exists(os.path.join(PKG, path)):
        subprocess.run(["make", "-C", PKG, path], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(PKG, path)], capture_output=True, text=True)
    assert r.returncode == 0 and "order_tables_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_the_export_and_the_flag(tmp_path):
    assert "ulg_order_search_table" in ulg.header_symbols() and hasattr(ulg.lib(), "ulg_order_search_table")
    tool = os.path.join(PKG, "bin", "ordersearch")
    run = lambda *a: subprocess.run([tool, *a], capture_output=True, text=True, timeout=60)  # noqa: E731
    assert "--tables" in run("--help").stdout
    missing = str(tmp_path / "none.pss")
    accepted, refused = run(missing, "--tables"), run(missing, "--tabels")
    assert accepted.returncode == 1 and "none.pss" in accepted.stderr  # parsed; the file is what fails
    assert refused.returncode == 2 and "tabels" in refused.stderr
