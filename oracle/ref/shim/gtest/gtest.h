// Stand-in for gtest: TEST(a, b) turns the test body into a function that nothing calls.
#pragma once

#define TEST(suite, name) [[maybe_unused]] static void suite##_##name##_never_called()
